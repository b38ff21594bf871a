"""GPU: the codebook quantiser (csrc/retrieval.hip) against exact expected indices at the shapes where each of its
branches runs.

The cases, their builder and the fp64 expectation are in tests/quantize_edge_cases.py; tests/test_quantize_edges_host.py
checks on the CPU that every query is separated by the margin (1e-3 against an emulated distance error of at most
2.3e-5), that a numpy restatement of the kernel's arithmetic selects exactly the expected indices, and that the cases
reach the branches they are meant to reach: the candidate-list overflow fallback (by ties and by tau = +inf in a short
tail block), the merge's fold of block lists beyond 256 blocks, every k template, k-step counts 1, 2, 5, 6, 7, 12, 13,
and one, two and three query groups with padded rows.

Every comparison is ``array_equal``: no near-tie tolerance, no share of allowed mismatches. Duplicated codebook rows
must tie bit-exactly and break to the lower row, inside a block, across blocks and across the merge's folded lists.

Mutation check (by hand on a copy, not committed; selection-only changes of retrieval.hip, of 44 tests):
  * the fallback without ``kmerge_xor<K>(L, 32)``: 17 red (the six tau = +inf tails and tails C = 45, 301, 300 k 7,
    ties k = 8 and 5, ksteps k = 7 and 8, plumb k = 8, the repeat test of ties, the workspace test);
  * ``rq_merge_kernel`` without its fold loop: 3 red (big k = 8 and 1, the repeat test of big);
  * ``d < tq`` in the filter: 36 red, every family;
  * ``tau[ql] = L[K - 2]`` for K > 1: 32 red, every family except big. It loses a block's k-th nearest row only when
    the block holds k of the query's k nearest in k different lane slots; the 321 blocks of big hold at most a few
    of them each, so big survives it (its three tests stay green), as do the three k = 1 cases, groups M = 1 and the
    tails C = 8, 25, 40, 44, 45 at k = 8.
"""
import numpy as np
import pytest
import torch

import quantize_edge_cases as E

pytestmark = pytest.mark.gpu


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the cases are read-only


_BOOKS = {}


def _book(cs):
    """One Codebook per distinct centroid array (cases of one seed share it)."""
    from m3s.retrieval import Codebook

    key = id(cs.c)
    if key not in _BOOKS:
        _BOOKS[key] = (cs.c, Codebook(_cuda(cs.c)))
    return _BOOKS[key][1]


def _run(cs, book=None, q=None):
    book = _book(cs) if book is None else book
    got = book.quantize(_cuda(cs.q) if q is None else q, cs.k).cpu().numpy()
    assert got.dtype == np.int64 and got.shape == cs.topk.shape
    return got


def _report(cs, got):
    bad = np.argwhere(got != cs.topk)
    return (f"{cs.name}: {len(bad)} of {got.size} indices differ; first (query, rank) {bad[:5].tolist()}, got "
            f"{[got[tuple(b)] for b in bad[:5]]}, expected {[cs.topk[tuple(b)] for b in bad[:5]]}")


@pytest.mark.parametrize("name", E.NAMES)
def test_case_exact_indices(name):
    cs = E.case(name)
    got = _run(cs)
    assert np.array_equal(got, cs.topk), _report(cs, got)


@pytest.mark.parametrize("family", ["ties", "big"])
def test_ties_repeat_and_k1_is_first_column(family):
    """The LDS list slots are handed out by atomics: the result must not depend on their order. The database-add
    assignment (k = 1) is the first column of the k = 8 assignment."""
    cs = E.case(f"{family}-k8")
    book, q = _book(cs), _cuda(cs.q)
    runs = [_run(cs, book, q) for _ in range(3)]
    assert np.array_equal(runs[0], cs.topk), _report(cs, runs[0])
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])
    one = E.case(f"{family}-k1")
    assert one.c is cs.c and np.array_equal(one.q, cs.q)
    got1 = _run(one, book, q)
    assert np.array_equal(got1[:, 0], runs[0][:, 0])
    if family == "ties":
        five = E.case("ties-k5")
        assert np.array_equal(_run(five, book, q), runs[0][:, :5])


@pytest.mark.parametrize("D,k", E.POW2)
@pytest.mark.parametrize("e", [12, -12])
def test_power_of_two_scale_changes_nothing(D, k, e):
    """Every operation of the kernel commutes with a power-of-two scale while nothing over- or underflows (values
    here stay within 2^-12 * 2^-9 * 1e-3 .. 2^24 * 2): the indices are the device's own unscaled ones, bit for bit."""
    from m3s.retrieval import Codebook

    cs = E.case(f"ksteps-D{D}-k{k}")
    base = _run(cs)
    s = np.float32(2.0 ** e)
    got = _run(cs, Codebook(_cuda(cs.c * s)), _cuda(cs.q * s))
    assert np.array_equal(got, base)
    assert np.array_equal(got, cs.topk), _report(cs, got)


def test_workspace_reuse_streams_and_views():
    """One Codebook run at (M, k) = (305, 8), (1, 1), (609, 2), (40, 8), so that the shared "quantize" workspace
    grows, is reused for a smaller call and grows again, interleaved with a Codebook of another (C, D); one call on a
    non-default stream; one call fed a transposed fp64 view. Every call returns what its case returns alone
    (test_case_exact_indices: the expectation)."""
    from m3s.retrieval import Codebook

    cases = [E.case(E.plumb_name(M, k)) for M, k in E.PLUMB]
    other = [E.case("ksteps-D224-k7"), E.case("tails-C45-k8"), E.case("ksteps-D224-k7"), E.case("ties-k8")]
    book = Codebook(_cuda(cases[0].c))
    assert all(np.array_equal(cs.c, cases[0].c) for cs in cases)
    for _ in range(2):
        for cs, ot in zip(cases, other):
            got = _run(cs, book)
            assert np.array_equal(got, cs.topk), _report(cs, got)
            got = _run(ot, Codebook(_cuda(ot.c)))
            assert np.array_equal(got, ot.topk), _report(ot, got)
    # a non-default stream: its own workspace, ordered after the inputs' uploads
    cs = cases[0]
    q = _cuda(cs.q)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out = book.quantize(q, cs.k)
    stream.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got, cs.topk), _report(cs, got)
    # a transposed, non-contiguous fp64 view of the queries
    cs = cases[3]
    qt = _cuda(np.ascontiguousarray(cs.q.T, dtype=np.float64)).T
    assert qt.shape == cs.q.shape and not qt.is_contiguous() and qt.dtype == torch.float64
    got = _run(cs, book, qt)
    assert np.array_equal(got, cs.topk), _report(cs, got)
    # and a numpy array on the host
    got = book.quantize(np.array(cases[1].q), cases[1].k).cpu().numpy()
    assert np.array_equal(got, cases[1].topk)
