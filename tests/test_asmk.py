"""The ASMK database (``m3s_asmk_*``, ``m3s.retrieval.AsmkDatabase``), the part that needs no GPU.

``tests/asmk_ref.py`` restates the update in numpy in the device's forward-file formulation. Here it reproduces every
array of ``tests/golden/asmk_update.npz``, which the reference's own ASMKKernel + IVF wrote: codes, words and lists
exactly, scores to the derived tolerance (every term non-negative and a few fp32 ulps from the reference's, fp64
sums: rtol 1e-6, atol 1e-12). That is what shows the forward file computes what the inverted file computes.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import asmk_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASMK_SYMBOLS = ("m3s_asmk_db_size", "m3s_asmk_db_init", "m3s_asmk_workspace_size", "m3s_asmk_aggregate",
                "m3s_asmk_search", "m3s_asmk_add", "m3s_asmk_update")


@pytest.mark.parametrize("name", R.CASES)
def test_forward_file_reproduces_reference_fixture(golden, name):
    g = golden("asmk_update.npz")
    case = R.load_case(g, name)
    db = R.ForwardDb(case["c"], case["kq"], case["kb"])
    for i in range(case["n"]):
        ids = case["ids"][i]
        for k in ((case["kq"], case["kb"]) if i > 0 else (case["kb"],)):
            R.assert_fixture_aggregate(g, name, i, k, *R.aggregate(case["feats"][i], ids[:, :k], case["c"]))
        inds, scores = db.update(case["feats"][i], ids, True, case["K"], case["min_thresh"], ids_build=ids)
        assert inds == case["lists"][i], (name, i)
        if i > 0:
            np.testing.assert_allclose(scores, g[f"{name}_scores{i}"], rtol=R.RTOL, atol=R.ATOL)
    assert db.n_images == case["n"] and db.img_ptr[-1] == len(db.words)


@pytest.mark.parametrize("name", R.CASES)
def test_fixture_word_ids_have_no_near_tie(golden, name):
    """The fixture stores the reference's fp32 word ids. A quantiser accurate to test_retrieval's TOL must assign the
    same ones: the first k + 1 fp64 distances of every feature are further apart than that."""
    import oracle.oracle as O

    from test_retrieval import TOL

    case = R.load_case(golden("asmk_update.npz"), name)
    for i in range(case["n"]):
        k = case["ids"][i].shape[1]
        idx, l2 = O.quantize_custom(case["c"], case["feats"][i], k)
        assert (idx == case["ids"][i]).all()
        near = np.sort(np.partition(l2, k, axis=1)[:, :k + 1], axis=1)
        assert np.diff(near, axis=1).min() > TOL


def test_library_exports_asmk_and_abi_version_agrees():
    from m3s import _lib

    header = open(os.path.join(REPO, "include", "m3s.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in ASMK_SYMBOLS:
        assert hasattr(lib, s) and s in _lib.EXPORTED and re.search(r"\b%s\s*\(" % s, header), s
    lib.m3s_abi_version.restype = ctypes.c_int
    assert lib.m3s_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define M3S_ABI_VERSION (\d+)", header).group(1))
    assert _lib.ABI_VERSION >= 8
    assert ctypes.sizeof(_lib.AsmkResult) == 4 + 4 * 64 + 4 + 8 * 64  # count, idx, padding, score


def test_sim_table_and_packing_conventions():
    tab = R.sim_table(96, 3.0, 0.0)
    assert tab.dtype == np.float32 and tab[0] == 1 and tab[48] == 0 and (tab[49:] == 0).all() and (tab[:48] > 0).all()
    assert R.sim_table(96, 3.0, 0.5)[24] == np.float32(0.5) ** 3 and R.sim_table(96, 3.0, 0.5)[25] == 0
    # dim d lands in word d // 32 at bit 31 - d % 32
    c = np.zeros((1, 64), np.float32)
    des = np.zeros((1, 64), np.float32)
    des[0, [0, 33]] = 1
    codes, words = R.aggregate(des, np.zeros((1, 1), np.int64), c)
    assert codes.tolist() == [[1 << 31, 1 << 30]] and words.tolist() == [0]
    assert R.popcount32(np.array([0, 1, 0xffffffff, 0x80000001], np.uint32)).tolist() == [0, 1, 32, 2]


def test_params_outside_the_built_family_raise():
    from m3s.retrieval import AsmkDatabase, asmk_config

    assert asmk_config(R.asmk_params(5, 1)) == (5, 1, 3.0, 0.0)
    assert asmk_config(R.asmk_params(4, 2, 2.5, 0.1, binary="bin")) == (4, 2, 2.5, 0.1)
    c = np.zeros((64, 96), np.float32)
    for bad, what in ((R.asmk_params(5, 1, use_idf=True), "use_idf"), (R.asmk_params(5, 1, binary=False), "binary"),
                      (R.asmk_params(5, 1, binary="nobin"), "binary"), (R.asmk_params(2, 3), "k_build"),
                      (R.asmk_params(9, 1), "k_query")):
        with pytest.raises(RuntimeError, match=what):
            asmk_config(bad)
        with pytest.raises(RuntimeError, match=what):  # raised before any device is touched
            AsmkDatabase(c, bad)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        AsmkDatabase(np.zeros((64, 48), np.float32), R.asmk_params(5, 1))


def test_abi_host_checks_reject_bad_shapes():
    from m3s import _lib

    lib = _lib.load(require_gpu=False)
    assert lib.m3s_asmk_db_size(96, 4, 100) > 0 and lib.m3s_asmk_db_size(1024, 512, 512 * 512) < 64 << 20
    assert lib.m3s_asmk_db_size(48, 4, 100) == 0  # D % 32 != 0
    assert lib.m3s_asmk_workspace_size(64, 96, 33, 3) > 0
    assert lib.m3s_asmk_workspace_size(64, 48, 33, 3) == 0  # D % 32 != 0
    assert lib.m3s_asmk_workspace_size(64, 96, 1000, 5) == 0  # M * k > 4096
    db = _lib.AsmkDb(buf=256, bytes=1 << 30, D=48, max_images=4, max_entries=100)  # rejected before buf is used
    with pytest.raises(RuntimeError, match="multiple of 32"):
        _lib.check(lib.m3s_asmk_db_init(db, 3.0, 0.0, None))
    p = ctypes.c_void_p(256)  # non-null stand-ins: every call below is rejected before a pointer is used

    def aggregate(C, D, M, k, use_cols):
        return lib.m3s_asmk_aggregate(p, C, D, p, M, p, k, use_cols, p, p, p, p, 1 << 30, None)

    for args, what in (((64, 48, 33, 3, 3), "multiple of 32"), ((64, 96, 1000, 5, 5), "4096"),
                       ((64, 96, 5000, 1, 1), "4096"), ((64, 96, 33, 3, 4), "use_cols"), ((64, 96, 33, 9, 1), "1..8"),
                       (((1 << 20) + 1, 96, 33, 3, 3), "2\\^20")):
        with pytest.raises(RuntimeError, match=what):
            _lib.check(aggregate(*args))
