"""tt_mlp_rows at layers wider than 384 (one launch over column groups)
against the same GEMM as ceil(N / 384) narrow launches on column slices of B
(the N <= 384 kernels, unchanged): the grouped launch in the library's own
choice of block order ("single") and in both orders forced
(TT_MLP_ROWS_ORDER), each replayed from a hipGraph between HIP events.  The
arms are timed interleaved, RUNS times; per arm the min, median and max are
printed, and whether the single launch is within the split form's own
min-max spread.  For information: torch fp32 mm (hipBLASLt) and the fraction
of the bf16x3 MFMA floor (3 v_mfma_f32_32x32x16_bf16 per 32 x 32 x 16 product
block, 32 cycles each per SIMD, 1024 SIMDs at a nominal 2.4 GHz).

usage: python tools/time_mlp_wide.py [M] [RUNS] [KxN | KxNm ...]
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hm-retrieval-two-tower_amd")]
import torch  # noqa: E402

from pkg.modelling import hip_ops  # noqa: E402

M = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
REPS = 50
dev = torch.device("cuda:0")
g = torch.Generator(device=dev)
g.manual_seed(0)


def capture(fn):
    """fn x REPS as one hipGraph (warmed)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
        for _ in range(REPS):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    return graph


def replay_us(graph):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


def floor_us(K, N):
    mfmas = 3 * ((M + 31) // 32) * ((N + 31) // 32) * ((K + 15) // 16)
    return mfmas * 32 / (1024 * 2.4e9) * 1e6


def layer(name, K, N, masked):
    ld = lambda n: (n + 3) // 4 * 4
    A = torch.randn(M, ld(K), generator=g, device=dev)[:, :K]
    out = torch.empty(M, ld(N), device=dev)[:, :N]
    if masked:  # input gradient: B = W^T of W [N, K], ReluGrad on A, the layer below's mask on C
        W = torch.randn(N, K, generator=g, device=dev) * K ** -0.5
        kw = dict(amask=torch.randn(M, ld(K), generator=g, device=dev)[:, :K], scale=torch.full((1,), 0.5, device=dev),
                  cmask=torch.randn(M, ld(N), generator=g, device=dev)[:, :N] if N % 4 == 0 else None)
        B = W.t()
    else:
        W = torch.randn(K, N, generator=g, device=dev) * K ** -0.5
        kw = dict(bias=torch.randn(N, generator=g, device=dev), relu=True)
        B = W
    img = hip_ops.mlp_pack(W, trans=masked)

    def single():
        hip_ops.mlp_rows(A, img, K, N, out, **kw)

    out_s = torch.empty(M, ld(N), device=dev)[:, :N]
    slices = []
    for j0 in range(0, N, 384):
        w = min(384, N - j0)
        kws = {k: (v[j0:j0 + w].contiguous() if k == "bias" else v[:, j0:j0 + w] if k == "cmask" and v is not None else v)
               for k, v in kw.items()}
        wj = W[j0:j0 + w] if masked else W[:, j0:j0 + w].contiguous()
        slices.append((hip_ops.mlp_pack(wj, trans=masked), w, out_s[:, j0:j0 + w], kws))

    def split():
        for im, w, o, kws in slices:
            hip_ops.mlp_rows(A, im, K, w, o, **kws)

    Bc = B.contiguous()
    out_t = torch.empty(M, N, device=dev)
    Ac = A.contiguous()
    arms = {}
    for order in ("xcd", "group"):
        os.environ["TT_MLP_ROWS_ORDER"] = order  # read by the library at every call, frozen into the capture
        arms["single/" + order] = capture(single)
    os.environ.pop("TT_MLP_ROWS_ORDER")
    arms["single"] = capture(single)  # the library's own choice of order
    single()
    split()
    torch.cuda.synchronize()
    assert torch.equal(out, out_s), "single launch != split form"
    arms["split"] = capture(split)
    arms["torch mm"] = capture(lambda: torch.mm(Ac, Bc, out=out_t))
    t = {k: [] for k in arms}
    for _ in range(RUNS):
        for k, gr in arms.items():
            t[k].append(replay_us(gr))
    fl = floor_us(K, N)
    print(f"{name}: M={M} K={K} N={N} {'masked' if masked else 'bias+relu'}; bf16x3 MFMA floor {fl:.1f} us")
    for k, v in t.items():
        frac = f", {fl / min(v):.0%} of floor" if k != "torch mm" else ""
        print(f"  {k:13s} min {min(v):7.1f}  med {statistics.median(v):7.1f}  max {max(v):7.1f} us{frac}")
    lo, hi = min(t["split"]), max(t["split"])
    for arm in ("single", "single/xcd", "single/group"):
        d = statistics.median(t[arm]) - statistics.median(t["split"])
        print(f"  {arm}: median {d:+.1f} us vs split (split spread {hi - lo:.1f} us) -> "
              f"{'ok' if d <= hi - lo else 'SLOWER than the split form by more than its spread'}")


layer("386->512 forward", 386, 512, False)
layer("512->512 forward", 512, 512, False)
layer("512->386 input gradient", 512, 386, True)
layer("1024->1024 forward", 1024, 1024, False)
for spec in sys.argv[3:]:  # further layers: KxN (forward) or KxNm (masked input gradient)
    k, n = spec.rstrip("m").split("x")
    layer(spec, int(k), int(n), spec.endswith("m"))
