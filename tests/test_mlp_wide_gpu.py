"""GPU: Dense layers wider than 384 (tt_mlp_rows / tt_mlp_rows_pair in column
groups, DenseStack(max_width=4096), Tower and TwoTowerModel at a 386-wide
input and [512] hidden layers).

The fp64 bound 2e-5 (relative 2-norm) is the project's bf16x3 bound
(test_kernels_gpu.test_mlp_rows_vs_torch_fp64).  The bit-identity tests run
the unchanged narrow kernel (N <= 384) on 128-aligned column windows of the
same problem: a wide launch must reproduce it exactly, so they pin the
arithmetic with no tolerance."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle
from pkg import dtypes
from pkg.modelling import hip_ops
from pkg.modelling.models.tower import DenseStack, backward_acts_pair, forward_acts_pair
from pkg.modelling.models.two_tower_model import GraphedTrainStep, TwoTowerModel
from pkg.modelling.optimizer_factory import OptimizerFactory
from pkg.schema.features import Feature, FeatureFamily

pytestmark = pytest.mark.gpu

# (M, K, N): the smallest shapes at which the column tiling can go wrong
SHAPES = [
    (130, 300, 385),    # first width past the limit; ragged N: scalar stores; 3 row blocks, the last ragged
    (130, 64, 512),     # two even groups
    (200, 37, 772),     # 7 units of 128: uneven groups, image blocks past NBp must not be touched
    (130, 520, 1152),   # exactly 3 x 384, K > 384
    (1, 5, 1153),       # M = 1, four groups, the last unit one ragged column
    (70, 48, 4096),     # the bound
]
WINDOWED = [s for s in SHAPES if s[2] <= 1153]
PAD = 8  # columns of the output buffers past ceil4(N): never written


def _ceil4(n):
    return (n + 3) // 4 * 4


@functools.lru_cache(maxsize=None)
def _case(M, K, N):
    """Operands of one shape and the wide kernel's results on them, computed
    once and shared (read-only) by the tests: forward form out = relu(A W + b),
    backward form out2 = (((Am > 0) A s) Wt^T) * (Cm > 0) with its column sums
    (cmask only when N % 4 == 0, as in DenseStack; called twice)."""
    cuda = torch.device("cuda:0")
    g = torch.Generator(device=cuda)
    g.manual_seed(M * 7 + K * 3 + N)
    lda, n4 = _ceil4(K), _ceil4(N)
    c = dict(M=M, K=K, N=N)
    c["A"] = torch.randn(M, lda, generator=g, device=cuda)[:, :K]
    c["W"] = torch.randn(K, N, generator=g, device=cuda) * K ** -0.5
    c["b"] = torch.randn(N, generator=g, device=cuda) * 0.1
    c["buf"] = torch.full((M, n4 + PAD), float("nan"), device=cuda)
    c["out"] = c["buf"][:, :N]
    hip_ops.mlp_rows(c["A"], hip_ops.mlp_pack(c["W"]), K, N, c["out"], bias=c["b"], relu=True)
    c["Wt"] = torch.randn(N, K, generator=g, device=cuda) * K ** -0.5
    c["Am"] = torch.randn(M, lda, generator=g, device=cuda)[:, :K]
    c["Cm"] = torch.randn(M, N + 4, generator=g, device=cuda)[:, :N] if N % 4 == 0 else None
    c["s"] = torch.full((1,), 0.75, device=cuda)
    c["buf2"] = torch.full((M, n4 + PAD), float("nan"), device=cuda)
    c["out2"] = c["buf2"][:, :N]
    c["cs"] = torch.full((N,), float("nan"), device=cuda)
    img = torch.empty(hip_ops.lib().tt_mlp_pack_bytes(K, N), dtype=torch.uint8, device=cuda)
    hip_ops.mlp_pack_many([(c["Wt"], True, img)])
    for _ in range(2):
        hip_ops.mlp_rows(c["A"], img, K, N, c["out2"], amask=c["Am"], scale=c["s"], cmask=c["Cm"], colsum=c["cs"])
    torch.cuda.synchronize()
    return c


def _rel(x, ref):
    return float((x.double() - ref).norm() / ref.norm().clamp_min(1e-30))


@pytest.mark.parametrize("M,K,N", SHAPES)
def test_wide_mlp_rows_vs_torch_fp64(cuda, M, K, N):
    """tt_mlp_rows at N > 384, forward and backward form, against torch fp64
    (2e-5); every output element written (the buffers start as NaN) and no
    column past ceil4(N) touched."""
    c = _case(M, K, N)
    n4 = _ceil4(N)
    A, out, out2 = c["A"], c["out"], c["out2"]
    ref = torch.relu(A.double() @ c["W"].double() + c["b"].double())
    assert torch.isfinite(out).all()
    err = _rel(out, ref)
    print(f"forward {M}x{K}x{N}: rel err {err:.2e}")
    assert err < 2e-5
    ref2 = (A.double() * (c["Am"] > 0).double() * 0.75) @ c["Wt"].double().t()
    if c["Cm"] is not None:
        ref2 = ref2 * (c["Cm"] > 0).double()
    assert torch.isfinite(out2).all()
    err2 = _rel(out2, ref2)
    print(f"backward {M}x{K}x{N}: rel err {err2:.2e}")
    assert err2 < 2e-5
    cs = c["cs"]
    assert torch.isfinite(cs).all()
    assert torch.allclose(cs.double(), out2.double().sum(0), rtol=1e-5, atol=1e-5 * float(out2.abs().sum(0).max()))
    for buf in (c["buf"], c["buf2"]):
        assert torch.isnan(buf[:, n4:]).all()  # beyond the row's padding: untouched
        pad = buf[:, N:n4]  # the row's own padding: zeros (vector stores) or left alone (scalar stores)
        assert bool(((pad == 0) | pad.isnan()).all())


@pytest.mark.parametrize("M,K,N", WINDOWED)
def test_wide_mlp_rows_windows_equal_narrow_kernel(cuda, M, K, N):
    """Every 128-aligned window of at most 384 columns of the wide result
    equals the narrow kernel on that slice of B, bias and cmask, written into
    the same columns of a second buffer — both forms and the column sums."""
    c = _case(M, K, N)
    A = c["A"]
    n4 = _ceil4(N)
    for j0 in range(0, N, 128):
        w = min(384, N - j0)
        buf = torch.full((M, n4 + PAD), float("nan"), device=cuda)
        view = buf[:, j0:j0 + w]
        hip_ops.mlp_rows(A, hip_ops.mlp_pack(c["W"][:, j0:j0 + w].contiguous()), K, w, view,
                         bias=c["b"][j0:j0 + w].contiguous(), relu=True)
        assert torch.equal(view, c["out"][:, j0:j0 + w]), ("forward", j0)
        img = torch.empty(hip_ops.lib().tt_mlp_pack_bytes(K, w), dtype=torch.uint8, device=cuda)
        hip_ops.mlp_pack_many([(c["Wt"][j0:j0 + w], True, img)])
        buf2 = torch.full((M, n4 + PAD), float("nan"), device=cuda)
        view2 = buf2[:, j0:j0 + w]
        cs = torch.full((w,), float("nan"), device=cuda)
        cm = c["Cm"][:, j0:j0 + w] if c["Cm"] is not None else None
        hip_ops.mlp_rows(A, img, K, w, view2, amask=c["Am"], scale=c["s"], cmask=cm, colsum=cs)
        assert torch.equal(view2, c["out2"][:, j0:j0 + w]), ("backward", j0)
        assert torch.equal(cs, c["cs"][j0:j0 + w]), ("colsum", j0)


@pytest.mark.parametrize("M,K,N", [(200, 37, 772),      # default order: XCD-chunked (image < 4 MiB)
                                   (130, 520, 1152),
                                   (130, 1024, 1024)])  # a 4 MiB image: group-major by default
def test_wide_mlp_rows_block_order_does_not_change_results(cuda, monkeypatch, M, K, N):
    """Both block orders of a grouped launch (TT_MLP_ROWS_ORDER=xcd / group;
    unset picks by the image size) run the same (row block, group) set:
    bit-identical outputs and column sums, within 2e-5 of fp64; any other
    value is refused."""
    c = _case(M, K, N)  # computed under the default order
    assert _rel(c["out"], torch.relu(c["A"].double() @ c["W"].double() + c["b"].double())) < 2e-5
    for order in ("xcd", "group"):
        monkeypatch.setenv("TT_MLP_ROWS_ORDER", order)
        out = torch.full((M, _ceil4(N)), float("nan"), device=cuda)[:, :N]
        hip_ops.mlp_rows(c["A"], hip_ops.mlp_pack(c["W"]), K, N, out, bias=c["b"], relu=True)
        assert torch.equal(out, c["out"]), order
        out2 = torch.full((M, _ceil4(N)), float("nan"), device=cuda)[:, :N]
        cs = torch.full((N,), float("nan"), device=cuda)
        hip_ops.mlp_rows(c["A"], hip_ops.mlp_pack(c["Wt"], trans=True), K, N, out2, amask=c["Am"], scale=c["s"],
                         cmask=c["Cm"], colsum=cs)
        assert torch.equal(out2, c["out2"]) and torch.equal(cs, c["cs"]), order
    monkeypatch.setenv("TT_MLP_ROWS_ORDER", "columns")
    with pytest.raises(hip_ops._native.TTError, match="TT_MLP_ROWS_ORDER"):
        hip_ops.mlp_rows(c["A"], hip_ops.mlp_pack(c["W"]), K, N, out, bias=c["b"], relu=True)


def _rows_problem(cuda, g, M, K, N, masked):
    lda = _ceil4(K)
    A = torch.randn(M, lda, generator=g, device=cuda)[:, :K]
    W = torch.randn(N, K, generator=g, device=cuda) * K ** -0.5 if masked else \
        torch.randn(K, N, generator=g, device=cuda) * K ** -0.5
    img = torch.empty(hip_ops.lib().tt_mlp_pack_bytes(K, N), dtype=torch.uint8, device=cuda)
    hip_ops.mlp_pack_many([(W, masked, img)])
    ldc = _ceil4(N)
    p = dict(a=A, img=img, k=K, n=N, out=torch.full((M, ldc), float("nan"), device=cuda)[:, :N])
    if masked:
        p.update(amask=torch.randn(M, lda, generator=g, device=cuda)[:, :K], scale=torch.full((1,), 0.5, device=cuda),
                 cmask=torch.randn(M, ldc, generator=g, device=cuda)[:, :N] if N % 4 == 0 else None)
    else:
        p.update(bias=torch.randn(N, generator=g, device=cuda), relu=True)
    return p


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shapes", [((130, 300, 512), (257, 64, 128)),    # wide + narrow
                                    ((64, 64, 772), (130, 128, 385)),     # 3 and 2 column groups
                                    ((257, 64, 128), (130, 300, 512))])   # narrow first
@pytest.mark.parametrize("order", [None, "group"])
def test_wide_mlp_rows_pair_equals_single(cuda, monkeypatch, shapes, masked, order):
    """tt_mlp_rows_pair with a wide problem (the flattened (problem, row block,
    group) grid, in either block order) is bit-identical to two tt_mlp_rows
    calls."""
    if order:
        monkeypatch.setenv("TT_MLP_ROWS_ORDER", order)
    g = torch.Generator(device=cuda)
    g.manual_seed(sum(sum(s) for s in shapes) + int(masked))
    probs = [_rows_problem(cuda, g, *s, masked) for s in shapes]
    hip_ops.mlp_rows_pair(probs)
    for p in probs:
        q = dict(p)
        single = torch.full_like(q["out"], float("nan"))
        q["out"] = single
        hip_ops.mlp_rows(q.pop("a"), q.pop("img"), q.pop("k"), q.pop("n"), q.pop("out"), **q)
        assert torch.isfinite(single).all()
        assert torch.equal(p["out"], single)


def _stack_run(cuda, in_dim, units, top_grad, M=1000):
    gen = torch.Generator()
    gen.manual_seed(in_dim + sum(units))
    st = DenseStack(in_dim, units, cuda, gen, max_width=4096)
    g = torch.Generator(device=cuda)
    g.manual_seed(in_dim * 3 + sum(units))
    x = torch.randn(M, _ceil4(in_dim), generator=g, device=cuda)[:, :in_dim]
    gout = torch.randn(M, units[-1], generator=g, device=cuda)
    s = torch.full((1,), 0.5, device=cuda) if top_grad else None
    return st, x, gout, s


@pytest.mark.parametrize("top_grad", [True, False])
@pytest.mark.parametrize("in_dim,units", [(386, [512, 128]),     # one more 128-d feature, a [512] hidden layer
                                          (130, [1024, 130]),    # wide hidden, odd top: padded wgrad beside a wide igrad
                                          (520, [384, 64])])     # only the input wide: the first layer's dx
def test_wide_dense_stack_vs_torch_fp64(cuda, in_dim, units, top_grad):
    """DenseStack(max_width=4096): forward against torch fp64, the flat
    gradient and dx against a torch fp64 backward that uses the GPU's own ReLU
    masks; 2e-5 each."""
    st, x, gout, s = _stack_run(cuda, in_dim, units, top_grad)
    flat = st.flat.detach()
    acts = st.forward_acts(x, flat)
    dx, gflat = st.backward_acts(acts, flat, gout.contiguous(), s, True)
    fd = flat.double()
    h = x.double()
    for w_off, fi, fo, b_off in st.layout:
        h = torch.relu(h @ fd[w_off:w_off + fi * fo].view(fi, fo) + fd[b_off:b_off + fo])
    e_f = _rel(acts[-1], h)
    ref = torch.zeros_like(fd)
    G = gout.double() * (0.5 if top_grad else 1.0) * (acts[-1] > 0).double()
    for li in range(len(st.layout) - 1, -1, -1):
        w_off, fi, fo, b_off = st.layout[li]
        ref[w_off:w_off + fi * fo] = (acts[li].double().t() @ G).reshape(-1)
        ref[b_off:b_off + fo] = G.sum(0)
        G = G @ fd[w_off:w_off + fi * fo].view(fi, fo).t()
        if li > 0:
            G = G * (acts[li] > 0).double()
    e_g, e_x = _rel(gflat, ref), _rel(dx, G)
    print(f"stack {in_dim}->{units}: forward {e_f:.2e}, flat gradient {e_g:.2e}, dx {e_x:.2e}")
    assert e_f < 2e-5 and e_g < 2e-5 and e_x < 2e-5


def test_wide_dense_stack_pair_equals_single(cuda):
    """forward_acts_pair / backward_acts_pair on two different wide stacks
    are bit-identical to each stack's own forward_acts / backward_acts."""
    runs = [_stack_run(cuda, 386, [512, 128], True, M=1000), _stack_run(cuda, 130, [1024, 128], True, M=700)]
    stacks = [r[0] for r in runs]
    flats = [st.flat.detach() for st in stacks]
    xs, gouts, s = [r[1] for r in runs], [r[2].contiguous() for r in runs], runs[0][3]
    acts = forward_acts_pair(stacks, xs, flats)
    pair = backward_acts_pair(stacks, acts, flats, gouts, s, [True, True])
    for t, st in enumerate(stacks):
        single = st.forward_acts(xs[t], flats[t])
        assert len(single) == len(acts[t])
        for a, b in zip(acts[t], single):
            assert torch.equal(a, b)
        dx, gflat = st.backward_acts(single, flats[t], gouts[t], s, True)
        assert torch.equal(pair[t][0], dx) and torch.equal(pair[t][1], gflat)
        assert torch.isfinite(dx).all() and torch.isfinite(gflat).all()


# --------------------------------------------------------------------------- model level
def _wide_model(cuda, seed=0):
    """Query input 128 + 128 + 130 = 386 wide, both towers [512] -> 32 (the
    two tables large enough to be sharded share one width, as the sharded
    step requires)."""
    V = [str(i) for i in range(300)]
    qf = [Feature("cust", dtypes.string, FeatureFamily.QUERY, embedding_size=128, vocab=V),
          Feature("post", dtypes.string, FeatureFamily.QUERY, embedding_size=128, vocab=V[:50]),
          Feature("freq", dtypes.string, FeatureFamily.QUERY, embedding_size=130, vocab=V[:20])]
    cf = [Feature("art", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=128, vocab=V),
          Feature("ptn", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=8, vocab=V[:20])]
    rng = np.random.default_rng(seed)
    probs = {str(i): float(p) for i, p in enumerate(rng.dirichlet(np.ones(300)))}
    m = TwoTowerModel(qf, cf, "art", 32, [512], [512], probs, device=cuda, seed=seed)
    m.compile(optimizer=OptimizerFactory.get_optimizer("adagrad", {"learning_rate": 0.05}))
    return m


def _wide_batch(cuda, rng, B):
    z = lambda v: torch.as_tensor((rng.zipf(1.3, B) % v).astype(np.int32), device=cuda)
    return {"cust": z(301), "post": z(51), "freq": z(21), "art": z(301), "ptn": z(21)}


def _assert_same_parameters(a, b):
    for ta, tb in zip(a.towers, b.towers):
        assert torch.equal(ta.dense.flat, tb.dense.flat)
        for n in ta.input_layer.embedding_layers:
            assert torch.equal(ta.input_layer.embedding_layers[n].weight, tb.input_layer.embedding_layers[n].weight), n


def _fp64_tower(tower, batch):
    with torch.no_grad():
        h = tower.input_layer(batch).double()
        for w, b in tower.dense.params():
            h = torch.relu(h @ w.detach().double() + b.detach().double())
    return h.cpu().numpy()


def test_wide_model_trains_eager_graphed_and_reloads(cuda, tmp_path):
    """A model the parent refuses to build (386-wide query input, [512] hidden
    layers), B = 512: the step-0 loss within 1e-3 relative of the fp64 loss
    (oracle.inbatch_softmax_xent on a torch fp64 forward of the towers; the
    bound test_c2_train_steps_match_cpu_restatement holds the default path to);
    three eager steps and the same steps through GraphedTrainStep on a twin
    train bit-identically; save / load reproduces the tower outputs exactly."""
    a, b = _wide_model(cuda, seed=4), _wide_model(cuda, seed=4)
    assert a.query_tower.input_layer.output_dim == 386
    assert [l[1:3] for l in a.query_tower.dense.layout] == [(386, 512), (512, 32)]
    assert [l[1:3] for l in a.candidate_tower.dense.layout] == [(136, 512), (512, 32)]
    rng = np.random.default_rng(11)
    batches = [_wide_batch(cuda, rng, 512) for _ in range(3)]
    ref = oracle.inbatch_softmax_xent(_fp64_tower(a.query_tower, batches[0]), _fp64_tower(a.candidate_tower, batches[0]),
                                      a.candidate_logq(batches[0]).cpu().numpy())["loss"]
    eager = [a.train_step(x)["loss"].clone() for x in batches]
    l0 = float(eager[0].item())
    print(f"step-0 loss {l0:.6f}, fp64 {ref:.6f}, rel {abs(l0 - ref) / abs(ref):.2e}")
    assert abs(l0 - ref) <= 1e-3 * abs(ref)
    g = GraphedTrainStep(b, batches[0], warmup=1)  # its warm-up step trains on batch 0
    graphed = [g.warmup_out["loss"].clone()] + [g(x)["loss"].clone() for x in batches[1:]]
    torch.cuda.synchronize()
    for i, (le, lg) in enumerate(zip(eager, graphed)):
        assert torch.isfinite(le).all() and torch.equal(le, lg), (i, le, lg)
    _assert_same_parameters(a, b)
    a.save(str(tmp_path / "model") + "/")
    r = TwoTowerModel.load(str(tmp_path / "model") + "/", device=cuda)
    for t0, t1 in zip(a.towers, r.towers):
        e0, e1 = t0(batches[2]), t1(batches[2])
        assert torch.isfinite(e0).all() and torch.equal(e0, e1)


def test_wide_model_world1_sharded_step_equals_graphed(cuda):
    """The world-1 sharded step (global negatives; the shortcut step and the
    one that runs its routed exchanges as real collectives on a one-rank
    group) on the wide model at B = 2048 trains bit-identically to the
    single-GPU GraphedTrainStep: 3 steps (call 1 eager, then graph replays)."""
    import socket

    import torch.distributed as dist

    from pkg.modelling.distributed import ShardedTrainStep, destroy_process_group

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device(cuda))
    try:
        a, b, c = (_wide_model(cuda, seed=8) for _ in range(3))
        xchg = ShardedTrainStep(a, shard_min_rows=300, global_negatives=True, always_exchange=True)
        short = ShardedTrainStep(b, shard_min_rows=300, global_negatives=True)
        assert xchg.use_graph and xchg.exchange and not short.exchange and xchg.tables is not None
        rng = np.random.default_rng(2048)
        batches = [_wide_batch(cuda, rng, 2048) for _ in range(3)]
        single = GraphedTrainStep(c, batches[0], warmup=1)  # its warm-up step trains on batch 0
        for i, batch in enumerate(batches):
            la, lb = xchg(batch)["loss"], short(batch)["loss"]
            lc = single.warmup_out["loss"] if i == 0 else single(batch)["loss"]
            assert torch.equal(la, lb) and torch.equal(la, lc), (i, la, lb, lc)
        assert xchg._graph is not None and short._graph is not None
        torch.cuda.synchronize()
        assert xchg._canary.tolist() == [0x7EADBEEF, 0, 0x7EADBEEF]
        for ta, tb, tc in zip(a.towers, b.towers, c.towers):
            assert torch.equal(ta.dense.flat, tb.dense.flat) and torch.equal(ta.dense.flat, tc.dense.flat)
            for name, t in tc.input_layer.embedding_layers.items():
                ma, mb = ta.input_layer.embedding_layers[name], tb.input_layer.embedding_layers[name]
                ga = xchg.tables.gather_full(ma._shard_key) if hasattr(ma, "_shard_key") else ma.weight
                gb = short.tables.gather_full(mb._shard_key) if hasattr(mb, "_shard_key") else mb.weight
                assert torch.equal(ga, gb) and torch.equal(ga, t.weight), name
        xchg.check_status()
        short.check_status()
    finally:
        destroy_process_group()  # the captured step graphs first, then the group
