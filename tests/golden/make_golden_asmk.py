"""Golden vectors of the ASMK database update, from the reference's own host code.

Runs only in the build container, where the reference tree exists (read-only); only the resulting
``asmk_update.npz`` is committed. What runs from the reference:

  mast3r_slam/retrieval_database.py  RetrievalDatabase.update, query, accumulate_scores, add_to_database,
                                     add_to_ivf_custom, quantize_custom: called unbound on a stand-in ``self`` whose
                                     prep_features returns the synthetic features
  asmk/kernel.py, inverted_file.py, functional.py, io_helpers.py   imported through a stub ``asmk`` package whose
                                     __path__ points into the reference tree (asmk_method / faiss are never imported)
  cython/hamming.pyx                 built into a scratch directory outside the repository

Stored per case: seed, shapes, an input checksum, the reference's word ids, per image the aggregated codes + words for
k_query and k_build (for D = 1024 the codes' sha256), the fp64 score vectors and the final ``update`` lists. Inputs
are regenerated from ``m3s.synthetic.asmk_sequence``.

Usage:  python tests/golden/make_golden_asmk.py
"""
import hashlib
import os
import subprocess
import sys
import sysconfig
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
ASMK = os.path.join(REF, "thirdparty", "mast3r", "asmk")
sys.dont_write_bytecode = True
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "lightweight-mast3r-slam_amd"), REPO):
    sys.path.insert(0, p)

import asmk_ref  # noqa: E402
import oracle.oracle as O  # noqa: E402
from m3s import synthetic  # noqa: E402

PARAMS = {"build_ivf": {"kernel": {"binary": True}, "ivf": {"use_idf": False},
                        "quantize": {"multiple_assignment": 1}, "aggregate": {}},
          "query_ivf": {"quantize": {"multiple_assignment": 5}, "aggregate": {}, "search": {"topk": None},
                        "similarity": {"similarity_threshold": 0.0, "alpha": 3.0}}}
#        name seed  C    D     M   k_query images
CASES = (("A", 21, 64, 96, 33, 3, 9),
         ("B", 22, 256, 128, 40, 5, 12),
         ("C", 23, 512, 1024, 300, 5, 6))
K, MIN_THRESH = 3, 5e-3  # config/base.yaml retrieval.k, retrieval.min_thresh
QUANT_TOL = 1e-4  # tests/test_retrieval.py TOL
SHA_FROM_D = 1024  # codes of this D and above are stored as sha256


def build_hamming(out_dir):
    c = os.path.join(out_dir, "hamming.c")
    subprocess.check_call([sys.executable, "-m", "cython", "-3", os.path.join(ASMK, "cython", "hamming.pyx"), "-o", c])
    so = os.path.join(out_dir, "hamming" + sysconfig.get_config_var("EXT_SUFFIX"))
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-I", sysconfig.get_paths()["include"], c, "-o", so])


def import_reference(scratch):
    build_hamming(scratch)
    pkg = types.ModuleType("asmk")
    pkg.__path__ = [os.path.join(ASMK, "asmk"), scratch]
    sys.modules["asmk"] = pkg
    for name in ("mast3r", "mast3r.retrieval", "mast3r.retrieval.processor", "mast3r.retrieval.model"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["mast3r.retrieval.processor"].Retriever = object
    sys.modules["mast3r.retrieval.model"].how_select_local = None
    sys.path.insert(0, REF)
    from asmk import inverted_file, io_helpers, kernel  # noqa: F401
    import mast3r_slam.retrieval_database as ref_rd

    return ref_rd, kernel, inverted_file


def make_database(ref_rd, kernel, inverted_file, centroids, params, log):
    """A stand-in ``self`` that runs the reference's RetrievalDatabase methods; aggregate_image and search record."""
    R = ref_rd.RetrievalDatabase
    codebook = types.SimpleNamespace(centroids=centroids)
    kern = kernel.ASMKKernel(codebook, **params["build_ivf"]["kernel"])
    ivf = inverted_file.IVF.initialize_empty(codebook_size=len(centroids), **params["build_ivf"]["ivf"])
    agg0, search0 = kern.aggregate_image, ivf.search

    def aggregate_image(des, word_ids):
        out = agg0(des, word_ids)
        log.append(("agg", word_ids.shape[1], out[0].copy(), out[1].copy()))
        return out

    def search(des, word_ids, **kw):
        ranks, ranked = search0(des, word_ids, **kw)
        scores = np.empty_like(ranked)
        scores[ranks] = ranked
        log.append(("scores", scores))
        return ranks, ranked

    kern.aggregate_image, ivf.search = aggregate_image, search

    class Db:
        update, query, accumulate_scores = R.update, R.query, R.accumulate_scores
        add_to_database, add_to_ivf_custom, quantize_custom = R.add_to_database, R.add_to_ivf_custom, R.quantize_custom

        def prep_features(self, feat):
            return feat

    db = Db()
    db.asmk = types.SimpleNamespace(params=params, codebook=codebook)
    db.ivf_builder = types.SimpleNamespace(kernel=kern, ivf=ivf, step_params=params["build_ivf"])
    db.kf_counter, db.kf_ids = 0, []
    db.query_dtype, db.query_device = torch.float32, "cpu"
    db.centroids = torch.from_numpy(centroids)
    return db


def gen_case(ref, name, seed, C, D, M, kq, n):
    params = {"build_ivf": PARAMS["build_ivf"], "query_ivf": dict(PARAMS["query_ivf"], quantize={"multiple_assignment": kq})}
    kb = params["build_ivf"]["quantize"]["multiple_assignment"]
    c, feats = synthetic.asmk_sequence(seed, C, D, M, n)
    log = []
    db = make_database(*ref, c, params, log)
    mine = asmk_ref.ForwardDb(c, kq, kb, **params["query_ivf"]["similarity"])
    out = {f"{name}_case": np.array([seed, C, D, M, kq, kb, n, K]), f"{name}_min_thresh": np.float64(MIN_THRESH),
           f"{name}_checksum": np.array([c.astype(np.float64).sum(), feats.astype(np.float64).sum()])}
    many_rows = empty_hit = False
    lists = []
    for i in range(n):
        del log[:]
        frame = types.SimpleNamespace(feat=torch.from_numpy(feats[i:i + 1]))
        inds = db.update(frame, True, K, MIN_THRESH)
        lists.append(inds)
        aggs = {k: (codes, words) for tag, k, codes, words in (e for e in log if e[0] == "agg")}
        # the word ids the reference quantised: k_query columns once an image is in, k_build for the first
        k_ids = kq if i > 0 else kb
        ids = R_quantize(ref[0], c, feats[i], k_ids)
        out[f"{name}_ids{i}"] = ids.astype(np.int32)
        # no near-tie among the first k + 1 fp64 distances: a quantiser within QUANT_TOL assigns the same words
        _, l2 = O.quantize_custom(c, feats[i], k_ids)
        near = np.sort(np.partition(l2, k_ids, axis=1)[:, :k_ids + 1], axis=1)
        assert np.diff(near, axis=1).min() > 2 * QUANT_TOL, (name, i, np.diff(near, axis=1).min())
        assert (O.quantize_custom(c, feats[i], k_ids)[0] == ids).all()
        for k, (codes, words) in aggs.items():
            my_codes, my_words = asmk_ref.aggregate(feats[i], ids[:, :k], c)
            assert (my_codes == codes).all() and (my_words == words).all(), (name, i, k)
            many_rows |= bool(((ids[:, :k, None] == words[None, None, :]).any(axis=1).sum(axis=0) >= 3).any())
            if D >= SHA_FROM_D:
                out[f"{name}_codes{i}_k{k}_sha256"] = np.frombuffer(
                    hashlib.sha256(np.ascontiguousarray(codes, dtype="<u4").tobytes()).digest(), dtype=np.uint8)
            else:
                out[f"{name}_codes{i}_k{k}"] = codes
            out[f"{name}_words{i}_k{k}"] = words.astype(np.int32)
        if i > 0:
            scores = [e[1] for e in log if e[0] == "scores"][0]
            out[f"{name}_scores{i}"] = scores
            assert (scores > 0).all(), (name, i)
            s = np.sort(scores)
            if len(s) > 1:
                assert (np.diff(s) / s[1:]).min() > 1e-4, (name, i, (np.diff(s) / s[1:]).min())
            empty_hit |= bool((~np.isin(aggs[kq][1], mine.words)).any())
        my_inds, my_scores = mine.update(feats[i], ids, True, K, MIN_THRESH, ids_build=ids)
        assert my_inds == inds, (name, i, my_inds, inds)
        if i > 0:
            np.testing.assert_allclose(my_scores, scores, rtol=1e-6, atol=1e-12)
            print(f"  {name} query {i}: {len(aggs[kq][1])} unique words, scores {scores.min():.2e} .. {scores.max():.2e}, "
                  f"list {inds}, max rel diff {np.abs(my_scores / scores - 1).max():.1e}")
    assert many_rows and empty_hit, (name, many_rows, empty_hit)
    assert any(lists), lists
    width = max(len(x) for x in lists)
    out[f"{name}_lists"] = np.array([x + [-1] * (width - len(x)) for x in lists], dtype=np.int32)
    return out


def R_quantize(ref_rd, c, feat, k):
    fake = types.SimpleNamespace(centroids=torch.from_numpy(c))
    return ref_rd.RetrievalDatabase.quantize_custom(fake, torch.from_numpy(feat),
                                                    {"quantize": {"multiple_assignment": k}}).numpy()


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as scratch:
        ref = import_reference(scratch)
        out = {}
        for case in CASES:
            print("case", case)
            out.update(gen_case(ref, *case))
    # min_thresh cuts some list short and leaves some whole
    cut = [(row >= 0).sum() < min(K, i) for name, *_ in CASES for i, row in enumerate(out[f"{name}_lists"]) if i > 0]
    assert any(cut) and not all(cut)
    path = os.path.join(HERE, "asmk_update.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
