"""CPU: ranking metrics on multi-item ground truth, everything but the kernel —
the numpy restatement (tests/rank_metrics_ref.py) against a naive loop and
known values, tt_rank_metrics' host validation, the discount tables, and
IndexRankingMetrics on the host (string) path with stub indices."""
import ctypes
import math

import numpy as np
import pytest
import torch

import rank_metrics_ref as ref
from pkg import _native
from pkg.modelling import hip_ops
from pkg.modelling.metrics import IndexRankingMetrics
from pkg.modelling.metrics.index_recall import IndexRecall
from pkg.modelling.metrics.ranking_metrics import host_rank_metrics

PAD = ref.PAD


# --------------------------------------------------------------------------- the restatement
HAND_CAND = np.array([[7, 3, 9, 3, 5, 7, 11, 2],        # repeated 3 and 7
                      [4, 4, 4, 1, PAD, PAD, PAD, PAD],  # repeats, padded tail
                      [1, 2, 3, 4, 5, 6, 7, 8],          # m = 0 row
                      [8, -1, 6, 8, 0, 6, 5, 30]], np.int32)
HAND_TRUTH = np.array([[3, 5, -1, 11, 3, 40],            # duplicate 3, padding in the middle, 40 absent
                       [4, PAD, 1, 1, -7, 4],
                       [-1, PAD, -1, -2 ** 31, PAD, -5],
                       [0, 6, 8, 99, 5, 30]], np.int32)
HAND_KS = [8, 1, 5, 3, 8]


def test_restatement_equals_the_naive_loop_on_a_hand_written_case():
    vals, hits, m = ref.rank_metrics(HAND_CAND, HAND_TRUTH, HAND_KS)
    assert m.tolist() == [4, 2, 0, 6]
    for q in range(4):
        nv, nh, nm = ref.naive(HAND_CAND[q], HAND_TRUTH[q], HAND_KS)
        assert nm == m[q]
        assert nh == hits[q].tolist()
        assert np.array_equal(np.array(nv, np.float32).view(np.int32), vals[q].view(np.int32)), q
    assert not vals[2].any() and not hits[2].any()
    assert hits[0].tolist() == [3, 0, 2, 1, 3]  # 3 at 2, 5 at 5, 11 at 7; the second 3 is not credited
    assert hits[1].tolist() == [2, 1, 2, 1, 2]
    # the package's host path states the same definitions
    pv, ph, pm = host_rank_metrics(HAND_CAND, HAND_TRUTH, HAND_KS)
    assert np.array_equal(pv.view(np.int32), vals.view(np.int32)) and np.array_equal(ph, hits)
    assert np.array_equal(pm, m)


def test_restatement_equals_the_naive_loop_on_random_rows():
    rng = np.random.default_rng(0)
    cand = rng.integers(-2, 25, (40, 17)).astype(np.int32)
    truth = rng.integers(-3, 25, (40, 6)).astype(np.int32)
    truth[::7] = -1
    ks = [17, 1, 12, 5]
    vals, hits, m = ref.rank_metrics(cand, truth, ks)
    for q in range(40):
        nv, nh, nm = ref.naive(cand[q], truth[q], ks)
        assert nm == m[q] and nh == hits[q].tolist()
        assert np.array_equal(np.array(nv, np.float32).view(np.int32), vals[q].view(np.int32)), q


def test_known_values():
    f = np.float32
    ks = [5, 1, 2, 4]
    vals, hits, m = ref.rank_metrics(np.array([[7, 3, 9, 3, 5]]), np.array([[3, 5, 11]]), ks)
    assert m[0] == 3 and hits[0].tolist() == [2, 0, 1, 1]  # c = [0, 1, 1, 1, 2]
    recall, ap, ndcg, rr = vals[0, 0]
    assert recall == f(2) / f(3)
    assert ap == (f(1) / f(2) + f(2) / f(5)) / f(3)
    assert rr == f(0.5)
    disc, idcg = ref.tables(5)
    assert ndcg == (disc[1] + disc[4]) / idcg[3]
    assert abs(float(ndcg) - (1 / math.log2(3) + 1 / math.log2(6)) / (1 + 1 / math.log2(3) + 0.5)) < 1e-6
    assert vals[0, 1].tolist() == [0, 0, 0, 0]                       # k = 1: no hit yet
    assert vals[0, 2].tolist() == [f(1) / f(3), f(0.5) / f(2), disc[1] / idcg[2], f(0.5)]  # min(m, k) = 2
    assert vals[0, 3, 1] == f(0.5) / f(3)


def test_discount_tables_are_the_restated_ones():
    for k_list in (1, 12, 4096):
        disc, idcg = hip_ops.rank_discount_tables(k_list)
        rd, ri = ref.tables(k_list)
        assert disc.dtype == np.float32 and idcg.dtype == np.float32
        assert np.array_equal(disc.view(np.int32), rd.view(np.int32))
        assert np.array_equal(idcg.view(np.int32), ri.view(np.int32))
    assert ri[0] == 0 and rd[0] == 1 and ri.shape == (4097,)


def test_restated_reduction_is_close_to_fsum_and_skips_unscored_queries():
    rng = np.random.default_rng(1)
    cand = rng.integers(0, 40, (700, 12)).astype(np.int32)
    truth = rng.integers(-1, 40, (700, 3)).astype(np.int32)
    truth[::9] = -1
    vals, hits, m = ref.rank_metrics(cand, truth, [12, 1])
    f64, i64, nv = ref.reduce_acc(vals, hits, m)
    assert nv[0] == int((m > 0).sum()) < 700
    for j in range(2):
        for c in range(4):
            want = math.fsum(float(v) for v in vals[m > 0, j, c])
            assert abs(f64[j, c] - want) <= 1e-12 * abs(want)
        assert i64[j, 0] == hits[:, j].sum() and i64[j, 1] == (hits[:, j] > 0).sum()
    again = ref.reduce_acc(vals[:100], hits[:100], m[:100], (f64, i64, nv))
    assert again[2][0] == nv[0] + int((m[:100] > 0).sum()) and (again[0] > f64).all()


# --------------------------------------------------------------------------- C ABI validation
def test_rank_metrics_host_validation():
    """Every call is rejected (or returns) on the host: no kernel is launched,
    so fake non-NULL pointers are never dereferenced."""
    lib = _native.lib()
    p = 64  # a non-NULL "pointer"

    def ok(**kw):
        base = dict(cand=p, ld_cand=100, k_list=100, truth=p, ld_truth=12, T=12, n=3, ks=[1, 12, 100], num_ks=None,
                    disc=p, idcg=p, vals=p, hits=p, m=None, f64=None, i64=None, nv=None)
        return dict(base, **kw)

    def call(a):
        ks = (ctypes.c_int32 * max(1, len(a["ks"])))(*a["ks"]) if a["ks"] is not None else None
        num_ks = a["num_ks"] if a["num_ks"] is not None else len(a["ks"])
        return lib.tt_rank_metrics(a["cand"], a["ld_cand"], a["k_list"], a["truth"], a["ld_truth"], a["T"], a["n"], ks,
                                   num_ks, a["disc"], a["idcg"], a["vals"], a["hits"], a["m"], a["f64"], a["i64"],
                                   a["nv"], None)

    def bad(word, **kw):
        assert call(ok(**kw)) == _native.TT_ERR_BAD_ARG, kw
        msg = lib.tt_last_error().decode()
        assert "tt_rank_metrics" in msg and word in msg, (kw, msg)

    bad("k_list", k_list=0, ks=[])
    bad("k_list", k_list=4097, ld_cand=5000)
    assert "4096" in lib.tt_last_error().decode()
    bad("T", T=0)
    bad("T", T=1025, ld_truth=2000)
    assert "1024" in lib.tt_last_error().decode()
    bad("num_ks", ks=[], num_ks=0)
    bad("num_ks", ks=[1] * 17)
    bad("ks", ks=None, num_ks=2)
    bad("ks", ks=[1, 0])
    bad("ks", ks=[101])
    bad("ld_cand", ld_cand=99)
    bad("ld_truth", ld_truth=11)
    bad("n_queries", n=-1)
    for name in ("cand", "truth", "disc", "idcg", "vals", "hits"):
        bad(name, **{name: None})
    for present in (("f64",), ("i64",), ("nv",), ("f64", "i64"), ("f64", "nv"), ("i64", "nv")):
        bad("acc", **{name: p for name in present})
    assert call(ok(n=0)) == _native.TT_OK
    assert call(ok(n=0, f64=p, i64=p, nv=p, m=p)) == _native.TT_OK
    assert call(ok(n=0, cand=None, truth=None, disc=None, idcg=None, vals=None, hits=None)) == _native.TT_OK
    assert call(ok(n=0, k_list=4096, ld_cand=4096, T=1024, ld_truth=1024, ks=[4096] * 16)) == _native.TT_OK
    with pytest.raises(_native.TTError):
        _native.check(call(ok(T=0)))


def test_hip_ops_rank_metrics_argument_checks():
    c, t = torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        hip_ops.rank_metrics(c, t, [1, 4])  # CPU tensors: libtt has no CPU path


# --------------------------------------------------------------------------- IndexRankingMetrics
NAMES = np.array([["a", "b", "c", "b"], ["d", "e", "f", "g"], ["h", "i", "j", "k"]], dtype=object)


def test_string_identifiers_take_the_host_path():
    m = IndexRankingMetrics(lambda queries: NAMES, [1, 4, 2])
    truth = [["b", "c", "zz", "b"], [], ["k"]]
    got = m({"customer_id": ["x", "y", "z"]}, truth)
    assert m.seen == 2 and m.skipped == 1 and m.total == 3
    f = np.float32
    ap0 = (f(1) / f(2) + f(2) / f(3)) / f(3)  # hits at 2 and 3 of m = 3
    assert got["map"][4] == (np.float64(ap0) + np.float64(f(0.25))) / 2
    assert got["recall"][4] == (np.float64(f(2) / f(3)) + 1.0) / 2
    assert got["mrr"][4] == (0.5 + 0.25) / 2 and got["mrr"][1] == 0.0
    assert got["hit_rate"] == {1: 0.0, 4: 1.0, 2: 0.5}
    assert got["precision"][4] == 3 / (4 * 2) and got["precision"][2] == 1 / (2 * 2)
    assert m.hits == {1: 0, 4: 3, 2: 1}
    disc, idcg = ref.tables(4)
    assert got["ndcg"][4] == (np.float64((disc[1] + disc[2]) / idcg[3]) + np.float64(disc[3] / idcg[1])) / 2
    assert set(got) == {"recall", "map", "ndcg", "mrr", "hit_rate", "precision"}
    # bytes, a [B] vector and an object array: one true id per query
    m2 = IndexRankingMetrics(lambda queries: NAMES, [4])
    r = m2({}, np.array([b"c", "nope", "h"], dtype=object))
    assert m2.seen == 3 and r["hit_rate"][4] == 2 / 3 and r["mrr"][4] == (np.float64(f(1) / f(3)) + 0 + 1) / 3
    m2.log_metric(epoch=1)
    assert IndexRankingMetrics(lambda queries: NAMES, [4]).metric["map"][4] == 0.0  # nothing seen yet
    with pytest.raises(ValueError):
        IndexRankingMetrics(lambda queries: NAMES, [5])({}, truth)  # k beyond the index's width


def test_host_path_equals_the_restatement_on_integers():
    rng = np.random.default_rng(2)
    cand = rng.integers(0, 30, (50, 12)).astype(np.int64)
    truth = rng.integers(-1, 30, (50, 5)).astype(np.int64)
    truth[::6] = -1
    ks = [12, 1, 5]
    m = IndexRankingMetrics(lambda queries: cand, ks)  # a CPU integer array: the host path
    got = m({}, torch.as_tensor(truth))
    vals, hits, mm = ref.rank_metrics(cand, truth, ks)
    n = int((mm > 0).sum())
    assert m.seen == n and m.skipped == 50 - n
    for j, k in enumerate(ks):
        for c, name in enumerate(("recall", "map", "ndcg", "mrr")):
            want = math.fsum(float(v) for v in vals[mm > 0, j, c]) / n
            assert abs(got[name][k] - want) <= 1e-12 * want
        assert got["hit_rate"][k] == (hits[:, j] > 0).sum() / n
        assert got["precision"][k] == hits[:, j].sum() / (k * n)
    ragged = [[int(v) for v in row if v >= 0] for row in truth]
    m3 = IndexRankingMetrics(lambda queries: cand, ks)
    assert m3({}, ragged) == got


def test_single_true_id_totals_equal_index_recall():
    rng = np.random.default_rng(3)
    cand = np.stack([rng.permutation(40)[:10] for _ in range(30)])  # duplicate-free lists
    names = np.array([[f"article-{v}" for v in row] for row in cand], dtype=object)
    true = np.array([f"article-{v}" for v in rng.integers(0, 40, 30)], dtype=object)
    ks = [1, 5, 10]
    a, b = IndexRankingMetrics(lambda queries: names, ks), IndexRecall(lambda queries: names, ks)
    ra, rb = a({}, true), b({}, true)
    assert a.hits == b.hits and a.seen == b.seen == 30
    assert ra["recall"] == rb and ra["hit_rate"] == rb


def test_exclusions_are_forwarded():
    seen = []

    def index(*args, **kwargs):
        seen.append((args, kwargs))
        return np.array([["a", "b"], ["c", "d"]], dtype=object)

    m = IndexRankingMetrics(index, [1, 2])
    queries = {"customer_id": ["x", "y"]}
    m(queries, [["b"], ["c", "d"]])
    assert seen[-1] == ((queries,), {})  # one positional argument, as IndexRecall
    r = m(queries, [["b"], ["c", "d"]], exclusions=[["a"], []])
    assert seen[-1] == ((queries,), {"exclusions": [["a"], []]})
    assert r["recall"][1] == 0.25 and r["recall"][2] == 1.0 and m.seen == 4
    m.update(queries, [[], []], exclusions=[[], []])
    assert m.seen == 4 and m.skipped == 2
