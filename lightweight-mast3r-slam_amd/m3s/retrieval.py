"""Retrieval codebook quantization on the MI355X matrix cores.

The hot op of the reference's ``RetrievalDatabase`` is ``quantize_custom``
(``/root/reference/mast3r_slam/retrieval_database.py:96-105``): the squared distances of the M local
features of a keyframe to every codebook centroid, ``(|q|^2 + |c|^2) - 2 q c^T``, and the indices of
the k nearest (``torch.topk(..., largest=False).indices``). It is called once per query
(``accumulate_scores``, ``:119``, k = ``multiple_assignment`` of ``query_ivf``) and once per database
add without a previous query (``add_to_ivf_custom``, ``:151-153``).

``Codebook`` arranges the centroids once for the matrix cores (the reference moves them to the device
once, ``:20-22``); ``Codebook.quantize`` is one asynchronous C call (``m3s_quantize``: fragment prep
of the queries, the fused GEMM + block top-k kernel, the final merge) on torch's current stream.
``QuantizeMixin`` gives a ``RetrievalDatabase`` subclass the drop-in ``quantize_custom``.

The rest of ``RetrievalDatabase.update`` (``:43-72``: ``ASMKKernel.aggregate_image``, ``IVF.search``, ``torch.topk``,
``IVF.add``, all host loops over ~1400 visual words in the reference) runs on the device too: ``AsmkDatabase`` keeps
the database as a forward file in device memory and ``update_features`` is one asynchronous C call
(``m3s_asmk_update``: quantise, aggregate + binarise, score, top-k, append) and one small readback.
``DatabaseMixin`` gives a ``RetrievalDatabase`` subclass the reference's ``update`` / ``query`` /
``add_to_database``. Feature extraction (``prep_features``, the retrieval model) stays the host class's.
"""
import ctypes

import torch

from m3s import _lib


class Codebook:
    """The (C, D) fp32 centroids, prepared once for ``m3s_quantize`` on their device."""

    def __init__(self, centroids, device=None):
        c = torch.as_tensor(centroids)
        device = torch.device(device) if device is not None else (c.device if c.is_cuda else torch.device("cuda"))
        c = c.to(device=device, dtype=torch.float32).contiguous()
        if c.dim() != 2 or c.shape[0] < 1 or c.shape[1] < 1:
            raise RuntimeError(f"codebook: centroids must be (C, D), got {tuple(c.shape)}")
        lib = _lib.load()
        _lib.require_cuda("codebook", c)
        self.centroids = c
        self.C, self.D = int(c.shape[0]), int(c.shape[1])
        nbytes = lib.m3s_codebook_size(self.C, self.D)
        self._buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _lib.check(lib.m3s_codebook_prepare(_lib.ptr(c), self.C, self.D, _lib.ptr(self._buf), nbytes,
                                            _lib.stream_ptr(device)))

    @property
    def device(self):
        return self.centroids.device

    def quantize(self, qvecs, k):
        """(M, k) int64 indices of the k nearest centroids per row of ``qvecs`` (ascending distance)."""
        lib = _lib.load()
        q = torch.as_tensor(qvecs)
        if q.dim() != 2 or q.shape[1] != self.D:
            raise RuntimeError(f"quantize: qvecs must be (M, {self.D}), got {tuple(q.shape)}")
        q = q.to(device=self.device, dtype=torch.float32).contiguous()
        M, k = int(q.shape[0]), int(k)
        out = torch.empty((M, k), dtype=torch.int64, device=self.device)
        if M == 0:
            return out
        if not 1 <= k <= 8 or k > self.C:
            raise RuntimeError(f"quantize: multiple_assignment k={k} must be in 1..min(8, C={self.C})")
        nbytes = lib.m3s_quantize_workspace_size(self.C, self.D, M, k)
        st = _lib.stream_ptr(self.device)
        ws = _lib.workspace("quantize", nbytes, self.device, st)
        _lib.check(lib.m3s_quantize(_lib.ptr(self._buf), self.C, self.D, _lib.ptr(q), M, k, _lib.ptr(out),
                                    _lib.ptr(ws), nbytes, st))
        return out


class QuantizeMixin:
    """Mix into the reference's ``RetrievalDatabase`` (before it in the bases) to route
    ``quantize_custom`` through the matrix-core kernel; ``self.centroids`` is used as the codebook."""

    def quantize_custom(self, qvecs, params):
        cb = getattr(self, "_m3s_codebook", None)
        if cb is None or cb.centroids.data_ptr() != self.centroids.data_ptr():
            cb = Codebook(self.centroids)
            self._m3s_codebook = cb
        k = params["quantize"]["multiple_assignment"]
        return cb.quantize(qvecs, k)


def quantize_custom(centroids, qvecs, params):
    """Functional form of ``RetrievalDatabase.quantize_custom`` (prepares the codebook per call)."""
    cb = centroids if isinstance(centroids, Codebook) else Codebook(centroids)
    return cb.quantize(qvecs, params["quantize"]["multiple_assignment"])


# ------------------------------------------------------------------------------------------------
# The device-resident ASMK database
# ------------------------------------------------------------------------------------------------
def asmk_config(params):
    """(k_query, k_build, alpha, similarity_threshold) of the reference's asmk params dict
    (``mast3r/retrieval/processor.py:91-96``). Only its family is built: binary kernel, no idf, unlimited search
    ``topk``; anything else raises (no fallback to the host implementation)."""
    build, query = params["build_ivf"], params["query_ivf"]
    binary = {"bin": True, "nobin": False}.get(build["kernel"]["binary"], build["kernel"]["binary"])
    if binary is not True:
        raise RuntimeError("asmk: only the binary kernel is built (build_ivf.kernel.binary must be True)")
    if build["ivf"]["use_idf"]:
        raise RuntimeError("asmk: use_idf=True is not built (build_ivf.ivf.use_idf must be False)")
    if query.get("search", {}).get("topk") is not None:
        raise RuntimeError("asmk: query_ivf.search.topk must be None (update ranks every database image)")
    k_query = int(query["quantize"]["multiple_assignment"])
    k_build = int(build["quantize"]["multiple_assignment"])
    if not 1 <= k_build <= k_query <= 8:
        raise RuntimeError(f"asmk: need 1 <= k_build ({k_build}) <= k_query ({k_query}) <= 8")
    sim = query["similarity"]
    return k_query, k_build, float(sim["alpha"]), float(sim["similarity_threshold"])


class AsmkDatabase:
    """The ASMK image database on the device (``m3s_asmk_*``): a forward file of (binary code, word) entries in
    insertion order with per-image entry offsets. ``update_features`` is ``RetrievalDatabase.update`` after
    ``prep_features``: one asynchronous C call on torch's current stream and one small readback. ``params`` is the
    reference's asmk params dict. The buffers grow geometrically when the C call reports the database full."""

    ENTRIES_PER_IMAGE = 512  # initial room per image (the workload adds <= 300); growth covers the rest

    def __init__(self, codebook_or_centroids, params, max_images=512):
        self.k_query, self.k_build, self.alpha, self.similarity_threshold = asmk_config(params)
        cb = codebook_or_centroids
        D = cb.D if isinstance(cb, Codebook) else (tuple(getattr(cb, "shape", ())) + (0, 0))[1]
        if D <= 0 or D % 32 != 0:
            raise RuntimeError(f"asmk: D={D} must be a positive multiple of 32 (the packed binary codes)")
        if int(max_images) < 1:
            raise RuntimeError("asmk: max_images must be positive")
        self.codebook = cb if isinstance(cb, Codebook) else Codebook(cb)
        self.C, self.D, self.W = self.codebook.C, self.codebook.D, self.codebook.D // 32
        self.device = self.codebook.device
        self._result = torch.zeros(ctypes.sizeof(_lib.AsmkResult), dtype=torch.uint8, device=self.device)
        self._n_scored = 0
        self._alloc(int(max_images), int(max_images) * self.ENTRIES_PER_IMAGE)

    # ---- buffers ----
    def _alloc(self, max_images, max_entries):
        lib = _lib.load()
        nbytes = lib.m3s_asmk_db_size(self.D, max_images, max_entries)
        if nbytes == 0:
            raise RuntimeError(f"asmk: database of {max_images} images / {max_entries} entries is too large")
        buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        db = _lib.AsmkDb(buf=buf.data_ptr(), bytes=nbytes, D=self.D, max_images=max_images, max_entries=max_entries)
        _lib.check(lib.m3s_asmk_db_init(db, self.alpha, self.similarity_threshold, _lib.stream_ptr(self.device)))
        self._buf, self._db = buf, db

    def _view(self, name, dtype, count):
        off = getattr(self._db, name) - self._db.buf
        return self._buf[off:off + count * dtype.itemsize].view(dtype)

    def _sections(self):
        db = self._db
        return (self._view("codes", torch.int32, db.max_entries * self.W).view(-1, self.W),
                self._view("words", torch.int32, db.max_entries), self._view("img_ptr", torch.int32, db.max_images + 1),
                self._view("norm", torch.int32, db.max_images))

    def _grow(self, need_entries):
        old, n, used = self._sections(), self._db.n_images, self._db.entries_bound
        max_images = self._db.max_images * 2 if n >= self._db.max_images else self._db.max_images
        max_entries = self._db.max_entries
        while used + need_entries > max_entries:
            max_entries *= 2
        self._alloc(max_images, max_entries)
        codes, words, img_ptr, norm = self._sections()
        codes[:used].copy_(old[0][:used])
        words[:used].copy_(old[1][:used])
        img_ptr[:n + 1].copy_(old[2][:n + 1])
        norm[:n].copy_(old[3][:n])
        self._db.n_images, self._db.entries_bound = n, used

    def _growing(self, call, need_entries):
        """Run ``call()`` (a C entry that adds an image); when it reports the database full, grow and repeat."""
        rc = call()
        if rc == _lib.ESPACE and b"database full" in _lib.load().m3s_last_error():
            self._grow(need_entries)
            rc = call()
        _lib.check(rc)

    @property
    def n_images(self):
        return int(self._db.n_images)

    def _features(self, feat):
        f = torch.as_tensor(feat)
        if f.dim() != 2 or f.shape[1] != self.D or f.shape[0] < 1:
            raise RuntimeError(f"asmk: features must be (M >= 1, {self.D}), got {tuple(f.shape)}")
        return f.to(device=self.device, dtype=torch.float32).contiguous()

    def _workspace(self, M, k):
        nbytes = _lib.load().m3s_asmk_workspace_size(self.C, self.D, M, k)
        if nbytes == 0:
            raise RuntimeError(f"asmk: M={M} features with {k} assignments exceed the 4096-key limit")
        st = _lib.stream_ptr(self.device)
        return _lib.workspace("asmk", nbytes, self.device, st), nbytes, st

    # ---- the three stages (m3s_asmk_aggregate / _search / _add) ----
    def aggregate(self, feat, word_ids, use_cols=None):
        """``ASMKKernel.aggregate_image`` of the first ``use_cols`` columns of ``word_ids`` (M, k): device tensors
        ``codes`` (M * use_cols, D / 32) int32 (the uint32 bit patterns), ``words`` (M * use_cols) int32 (sorted) and
        ``count`` (1) int32; the first ``count`` rows are valid."""
        lib = _lib.load()
        f = self._features(feat)
        ids = torch.as_tensor(word_ids).to(device=self.device, dtype=torch.int64).contiguous()
        M, k = int(f.shape[0]), int(ids.shape[1]) if ids.dim() == 2 else 0
        if ids.dim() != 2 or ids.shape[0] != M:
            raise RuntimeError(f"asmk aggregate: word_ids must be ({M}, k), got {tuple(ids.shape)}")
        use_cols = k if use_cols is None else int(use_cols)
        ws, nbytes, st = self._workspace(M, k)
        rows = M * max(use_cols, 1)
        codes = torch.empty((rows, self.W), dtype=torch.int32, device=self.device)
        words = torch.empty(rows, dtype=torch.int32, device=self.device)
        count = torch.empty(1, dtype=torch.int32, device=self.device)
        _lib.check(lib.m3s_asmk_aggregate(_lib.ptr(self.codebook.centroids), self.C, self.D, _lib.ptr(f), M,
                                          _lib.ptr(ids), k, use_cols, _lib.ptr(codes), _lib.ptr(words),
                                          _lib.ptr(count), _lib.ptr(ws), nbytes, st))
        return codes, words, count

    def search(self, codes, words, count):
        """``IVF.search`` of an aggregated query: the (n_images) float64 scores (device)."""
        lib = _lib.load()
        _lib.require_cuda("asmk search", codes, words, count)
        scores = torch.empty(self.n_images, dtype=torch.float64, device=self.device)
        _lib.check(lib.m3s_asmk_search(self._db, _lib.ptr(codes), _lib.ptr(words), _lib.ptr(count),
                                       int(words.shape[0]), _lib.ptr(scores), _lib.stream_ptr(self.device)))
        return scores

    def add(self, codes, words, count):
        """``IVF.add`` of one aggregated image under the next image id."""
        lib = _lib.load()
        _lib.require_cuda("asmk add", codes, words, count)
        rows = int(words.shape[0])
        st = _lib.stream_ptr(self.device)
        self._growing(lambda: lib.m3s_asmk_add(self._db, _lib.ptr(codes), _lib.ptr(words), _lib.ptr(count), rows, st),
                      rows)

    # ---- the fused update (m3s_asmk_update) ----
    def update_features(self, feat, add_after_query=True, k=3, min_thresh=0.0):
        """``RetrievalDatabase.update`` after ``prep_features`` for the (M, D) local features of one frame: the ids
        of the at most ``k`` best database images scoring above ``min_thresh`` (best first, ties by lower id), then
        the frame is added under the next id when ``add_after_query``. ``[]`` on an empty database."""
        lib = _lib.load()
        f = self._features(feat)
        M, n = int(f.shape[0]), self.n_images
        ws, nbytes, st = self._workspace(M, self.k_query)
        self._growing(lambda: lib.m3s_asmk_update(
            _lib.ptr(self.codebook._buf), _lib.ptr(self.codebook.centroids), self.C, self._db, _lib.ptr(f), M,
            self.k_query, self.k_build, int(k), float(min_thresh), int(bool(add_after_query)), _lib.ptr(self._result),
            _lib.ptr(ws), nbytes, st), M * self.k_build)
        self._n_scored = n
        if n == 0:
            self.last_scores = []
            return []
        res = _lib.AsmkResult.from_buffer_copy(self._result.cpu().numpy().tobytes())  # the one readback
        self.last_scores = list(res.score[:res.count])
        return list(res.idx[:res.count])

    def scores(self):
        """The float64 scores of every image the last ``update_features`` queried (a device copy)."""
        return self._view("scores", torch.float64, self._db.max_images)[:self._n_scored].clone()

    def export(self):
        """``(codes (E, D / 32) uint32, words (E) int32, img_ptr (n_images + 1) int32)`` as numpy arrays."""
        codes, words, img_ptr, _ = self._sections()
        img_ptr = img_ptr[:self.n_images + 1].cpu().numpy()
        E = int(img_ptr[-1])
        return codes[:E].cpu().numpy().view("uint32"), words[:E].cpu().numpy(), img_ptr


class DatabaseMixin(QuantizeMixin):
    """Mix into the reference's ``RetrievalDatabase`` (before it in the bases) to run ``update``, ``query`` and
    ``add_to_database`` on the device database. The host class supplies ``prep_features``, ``centroids`` and the asmk
    params (``self.asmk.params``); ``kf_counter`` and ``kf_ids`` are kept as the reference keeps them, and
    ``ivf_builder`` is never touched."""

    def _m3s_database(self):
        db = getattr(self, "_m3s_asmk_db", None)
        if db is None or db.codebook.centroids.data_ptr() != self.centroids.data_ptr():
            cb = getattr(self, "_m3s_codebook", None)
            if cb is None or cb.centroids.data_ptr() != self.centroids.data_ptr():
                cb = Codebook(self.centroids)
                self._m3s_codebook = cb
            db = AsmkDatabase(cb, self.asmk.params)
            self._m3s_asmk_db = db
        return db

    def update(self, frame, add_after_query, k, min_thresh=0.0):
        feat = self.prep_features(frame.feat)
        inds = self._m3s_database().update_features(feat[0], add_after_query, k, min_thresh)  # one frame at a time
        if add_after_query:
            self._m3s_bookkeep()
        return inds

    def _m3s_bookkeep(self):
        import numpy as np

        self.kf_ids.append(np.int64(self.kf_counter))
        self.kf_counter += 1

    def query(self, feat, id=None):
        """``(ranks (1, n), ranked scores (1, n), topk word ids (M, k_query))`` as numpy arrays, like the reference."""
        db = self._m3s_database()
        ids = db.codebook.quantize(db._features(feat), db.k_query)
        scores = db.search(*db.aggregate(feat, ids)).cpu().numpy()
        ranks = (-scores).argsort(kind="stable")
        return ranks[None], scores[ranks][None], ids.cpu().numpy()

    def add_to_database(self, feat_np, id_np, topk_codes=None):
        db = self._m3s_database()
        ids = topk_codes if topk_codes is not None else db.codebook.quantize(db._features(feat_np), db.k_build)
        db.add(*db.aggregate(feat_np, ids, db.k_build))
        self._m3s_bookkeep()
