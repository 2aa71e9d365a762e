"""The in-batch loss's ten *_workspace_size functions against a literal table
(recorded from the library before its host code was folded into one path per
pass): the fp32-prepared path (tt_inbatch_prep on two streams, then
..._prepped) and captured graphs rely on every size and carve staying where it
is.  n = 129 separates the square plan from the rectangular one, n = 5000 has a
split capped neither by the tiles nor by 16, dim 30 takes the scalar prep
path.  No GPU."""
import pytest

from pkg import _native

RECT = [(1, 1, 1), (100, 137, 30), (200, 448, 64), (129, 129, 128), (137, 100, 64), (16384, 16384, 128)]
FUSED_N = [1, 64, 100, 129, 5000, 16384]
DIMS = [30, 64, 128]
MIXED_M = [0, 37, 200]


def _arguments(name):
    """Every pinned call of one function, in the order of its row of PINNED."""
    if name in ("tt_inbatch_workspace_size", "tt_inbatch_x3_workspace_size"):
        return list(RECT)
    if name in ("tt_inbatch_hits_workspace_size", "tt_inbatch_hard_workspace_size",
                "tt_inbatch_mixed_workspace_size"):
        return [(*r, x3) for r in RECT for x3 in (0, 1)]
    if name in ("tt_inbatch_fused_workspace_size", "tt_inbatch_fused_x3_workspace_size"):
        return [(n, d) for n in FUSED_N for d in DIMS]
    if name in ("tt_inbatch_fused_hits_workspace_size", "tt_inbatch_fused_hard_workspace_size"):
        return [(n, d, x3) for n in FUSED_N for d in DIMS for x3 in (0, 1)]
    assert name == "tt_inbatch_fused_mixed_workspace_size"
    return [(n, m, d, x3) for n in FUSED_N for d in DIMS for x3 in (0, 1) for m in MIXED_M]


PINNED = {
    "tt_inbatch_fused_hard_workspace_size": [
        86016, 102400, 167936, 200704, 331776, 397312, 86016, 102400, 167936,
        200704, 331776, 397312, 86016, 102400, 167936, 200704, 331776, 397312,
        307200, 339968, 602112, 667648, 1191936, 1323008, 18309120, 18964480, 36003840,
        37314560, 71393280, 74014720, 19660800, 21757952, 38535168, 42729472, 76283904, 84672512,
    ],
    "tt_inbatch_fused_hits_workspace_size": [
        85504, 101888, 167424, 200192, 331264, 396800, 85504, 101888, 167424,
        200192, 331264, 396800, 85504, 101888, 167424, 200192, 331264, 396800,
        306176, 338944, 601088, 666624, 1190912, 1321984, 18288640, 18944000, 35983360,
        37294080, 71372800, 73994240, 19595264, 21692416, 38469632, 42663936, 76218368, 84606976,
    ],
    "tt_inbatch_fused_mixed_workspace_size": [
        86016, 86016, 130048, 102400, 102400, 154624, 167936, 167936, 252928,
        200704, 200704, 302080, 331776, 331776, 498688, 397312, 397312, 596992,
        86016, 86016, 173056, 102400, 102400, 205824, 167936, 167936, 336896,
        200704, 200704, 402432, 331776, 331776, 664576, 397312, 397312, 795648,
        86016, 145408, 222208, 102400, 169984, 254976, 167936, 284672, 435200,
        200704, 333824, 500736, 331776, 563200, 861184, 397312, 661504, 992256,
        307200, 307200, 402432, 339968, 339968, 443392, 602112, 602112, 787456,
        667648, 667648, 869376, 1191936, 1191936, 1557504, 1323008, 1323008, 1721344,
        18309120, 18309120, 18531328, 18964480, 18964480, 19194880, 36003840, 36003840, 36447232,
        37314560, 37314560, 37774336, 71393280, 71393280, 72279040, 74014720, 74014720, 74933248,
        19660800, 19735552, 19810304, 21757952, 21840896, 21923840, 38535168, 38683648, 38832128,
        42729472, 42894336, 43059200, 76283904, 76579840, 76875776, 84672512, 85001216, 85329920,
    ],
    "tt_inbatch_fused_workspace_size": [
        84992, 166912, 330752, 84992, 166912, 330752, 84992, 166912, 330752,
        305152, 600064, 1189888, 18268160, 35962880, 71352320, 19529728, 38404096, 76152832,
    ],
    "tt_inbatch_fused_x3_workspace_size": [
        101376, 199680, 396288, 101376, 199680, 396288, 101376, 199680, 396288,
        337920, 665600, 1320960, 18923520, 37273600, 73973760, 21626880, 42598400, 84541440,
    ],
    "tt_inbatch_hard_workspace_size": [
        31744, 44032, 98304, 122880, 647168, 745472, 518656, 633344, 188416,
        237568, 42795008, 51183616,
    ],
    "tt_inbatch_hits_workspace_size": [
        30720, 43008, 96256, 120832, 643072, 741376, 516608, 631296, 186368,
        235520, 42663936, 51052544,
    ],
    "tt_inbatch_mixed_workspace_size": [
        31744, 44032, 98304, 122880, 647168, 745472, 518656, 633344, 188416,
        237568, 42795008, 51183616,
    ],
    "tt_inbatch_workspace_size": [
        29952, 94720, 640000, 514816, 184832, 42532864,
    ],
    "tt_inbatch_x3_workspace_size": [
        42240, 119296, 738304, 629504, 233984, 50921472,
    ],
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_workspace_sizes_are_pinned(name):
    fn = getattr(_native.lib(), name)
    args = _arguments(name)
    assert len(args) == len(PINNED[name])
    got = [fn(*a) for a in args]
    wrong = [(a, g, w) for a, g, w in zip(args, got, PINNED[name]) if g != w]
    assert not wrong, f"{name}: (arguments, got, pinned) {wrong[:5]}"


def test_every_workspace_size_function_is_pinned():
    sizes = {s for s in _native.EXPORTED_SYMBOLS if s.startswith("tt_inbatch") and s.endswith("_workspace_size")}
    assert sizes == set(PINNED) and len(sizes) == 10


def test_unsupported_arguments_give_zero():
    lib = _native.lib()
    for name in PINNED:
        fn = getattr(lib, name)
        square = "fused" in name and "mixed" not in name  # (n, dim[, x3]); every other form has dim third
        for a in _arguments(name)[-2:]:
            bad_dim = list(a)
            bad_dim[1 if square else 2] = 300
            assert fn(*bad_dim) == 0, (name, bad_dim)
            assert fn(0, *a[1:]) == 0, (name, "n = 0")
    assert lib.tt_inbatch_workspace_size(16, 0, 64) == 0
    for x3 in (0, 1):
        assert lib.tt_inbatch_fused_mixed_workspace_size(100, -1, 64, x3) == 0
        assert lib.tt_inbatch_fused_mixed_workspace_size(0, -1, 64, x3) == 0
