"""The large-grid CPG forward (dvcp_cpg_tiled, 12 <= G <= 32; csrc/cpg_tiled.hip) against the CPU
oracle (oracle/ref_r.py cpg, plain nn.Conv3d), from the kernel up to dvcp.DeepVCP.

Inputs follow test_gpu_kernels.py::test_cpg_vs_oracle (the same generator pattern, O.cpg() weights
loaded into dvcp.cpg()).  Grids come from s = 0.25, so every int(2r/s + 1) is exact in binary.
The kernel's blocks: conv1 per axis ceil(G / 11) blocks of ceil(G / blocks) cells, conv2/conv3
ceil(G / 9) blocks, the edges the issue plans -- 12: two blocks per axis in both launches; 13: odd C,
unequal blocks (7 + 6); 17: 9 + 8; 23: three blocks (8 + 8 + 7: an interior block, a shorter last
one) in both launches; 32: the cap, 11 + 11 + 10 for conv1 and four blocks of 8 (two interior) for
conv2."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

S = 0.25
R_OF = {1: 0.0, 2: 0.125, 6: 0.625, 11: 1.25, 12: 1.375, 13: 1.5, 17: 2.0, 23: 2.75, 32: 3.875}
assert all(int((2 * r) / S + 1) == G for G, r in R_OF.items())   # (also in test_cpg_tiled_host.py)


def _inputs(G, B, K):
    g = torch.Generator().manual_seed(111)
    C = G ** 3
    src = torch.randn(B, K, 1, 32, generator=g)
    tgt = torch.randn(B, K, C, 32, generator=g).permute(0, 1, 3, 2)   # the reference's permuted view
    cand = torch.randn(B, K, C, 3, generator=g)
    return src, tgt, cand


def _oracle_module():
    import oracle as O
    torch.manual_seed(6)
    return O.cpg()


def _run_oracle(ref, src, tgt, cand, G):
    import oracle as O
    with torch.no_grad(), O.tracing() as tr:
        want = ref(src, tgt, cand, R_OF[G], S)
    return want, dict(tr)["cpg_weight"]


@functools.lru_cache(maxsize=None)
def _case(G, B=1, K=3):
    """One oracle run per grid, shared by the tests (read-only): (ref, src, tgt, cand, vcp, weights)."""
    ref = _oracle_module()
    src, tgt, cand = _inputs(G, B, K)
    want, w = _run_oracle(ref, src, tgt, cand, G)
    return ref, src, tgt, cand, want, w


def _mine(ref, cuda):
    import dvcp
    mine = dvcp.cpg().eval()
    mine.load_state_dict(ref.state_dict())
    return mine.to(cuda)


def _logits(ref, src, tgt, G):
    """The oracle's logits (cpg.py:27-52 up to the softmax), in the module's dtype."""
    nb, nk = src.shape[:2]
    cost = torch.square(src.reshape(nb, nk, 1, 1, 1, 32) - tgt.reshape(nb, nk, G, G, G, 32))
    x = cost.permute(0, 1, 5, 2, 3, 4).flatten(start_dim=0, end_dim=1)
    with torch.no_grad():
        return ref.conv3(ref.conv2(ref.conv1(x))).reshape(nb, nk, G ** 3)


@pytest.mark.parametrize("G", [12, 13, 17, 23, 32])
def test_cpg_large_grid_vs_oracle(cuda, G):
    """The module call on grids above 11^3 at the CPG's bar: vcp rtol/atol 1e-5, softmax weights
    rtol 1e-4 / atol 1e-7.  (Before dvcp_cpg_tiled this raised dvcp_cpg's "grid side" error.)"""
    from dvcp import ops
    assert ops.cpg_method(G) == "tiled"
    ref, src, tgt, cand, want, want_w = _case(G)
    mine = _mine(ref, cuda)
    got, w = mine(src.to(cuda), tgt.to(cuda), cand.to(cuda), R_OF[G], S, return_weights=True)
    print(f"cpg tiled G={G}: max|vcp err| {float((got.cpu() - want).abs().max()):.2e}, "
          f"max|w err| {float((w.cpu() - want_w).abs().max()):.2e} (max w {float(want_w.max()):.2e})")
    torch.testing.assert_close(got.cpu(), want, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(w.cpu(), want_w, rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("G", [1, 2, 6, 11])
def test_cpg_tiled_small_grids_match_lds_kernel(cuda, G):
    """method="tiled" forced at the one-workgroup kernel's grids: both paths against each other
    and against the oracle (not bit-equal: the summation order differs)."""
    from dvcp import ops
    ref, src, tgt, cand, want, want_w = _case(G, 2, 3)
    params = _mine(ref, cuda).packed_params()
    args = (src.to(cuda), tgt.to(cuda), cand.to(cuda), G, params)
    assert ops.cpg_method(G) == "lds"
    lds, lds_w = ops.cpg(*args, want_weight=True)
    til, til_w = ops.cpg(*args, want_weight=True, method="tiled")
    print(f"cpg G={G}: tiled vs lds max|vcp| {float((til - lds).abs().max()):.2e}, "
          f"max|w| {float((til_w - lds_w).abs().max()):.2e}")
    torch.testing.assert_close(til, lds, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(til_w, lds_w, rtol=1e-4, atol=1e-7)
    for v, w in ((lds, lds_w), (til, til_w)):
        torch.testing.assert_close(v.cpu(), want, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(w.cpu(), want_w, rtol=1e-4, atol=1e-7)


def test_cpg_tiled_target_layouts(cuda):
    """G = 13 with the target given as the permuted view of (B, K, C, 32) (the forward's), as a
    contiguous (B, K, 32, C) tensor, and as a batch slice whose stride(0) != K * stride(1)."""
    G, B, K = 13, 2, 3
    C = G ** 3
    ref, src, tgt, cand, want, want_w = _case(G, B, K)
    mine = _mine(ref, cuda)
    view = tgt.to(cuda)
    assert view.stride(2) == 1 and view.stride(3) == 32
    dense = view.contiguous()
    assert dense.stride(2) == C and dense.stride(3) == 1
    wide = torch.zeros(B, K + 1, 32, C, device=cuda)
    wide[:, :K] = view
    sliced = wide[:, :K]
    assert sliced.stride(0) != K * sliced.stride(1)
    for name, t in (("permuted view", view), ("contiguous", dense), ("batch slice", sliced)):
        got, w = mine(src.to(cuda), t, cand.to(cuda), R_OF[G], S, return_weights=True)
        print(f"cpg tiled G={G} {name}: max|vcp err| {float((got.cpu() - want).abs().max()):.2e}")
        torch.testing.assert_close(got.cpu(), want, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(w.cpu(), want_w, rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("variant", ["bias+100", "weight*50"])
@pytest.mark.parametrize("G", [12, 23])
def test_cpg_tiled_softmax_range(cuda, G, variant):
    """Logits far from 0: conv3.bias + 100 (every logit above exp's fp32 overflow at 88.7 unless
    the key point's global maximum is subtracted across blocks) and conv3.weight x 50 (a span of
    150 and more).  The fp32 oracle itself is further than 1e-5 from exact arithmetic here, so
    the reference is the fp64 oracle and the bar 1e-5 + 4 max|fp32 oracle - fp64 oracle|: the GPU's
    error is of the fp32 oracle's own kind (another summation order, plus the split's dropped terms
    of one rounding each), so the same order of magnitude is the honest bound."""
    import oracle as O
    _, src, tgt, cand, _, _ = _case(G)
    ref = _oracle_module()
    with torch.no_grad():
        if variant == "bias+100":
            ref.conv3.bias += 100.0
        else:
            ref.conv3.weight *= 50.0
    lg = _logits(ref, src, tgt, G)
    span = float((lg.max(-1).values - lg.min(-1).values).max())
    print(f"cpg tiled G={G} {variant}: max logit {float(lg.max()):.1f}, max |logit| {float(lg.abs().max()):.1f}, "
          f"span {span:.1f}")
    if variant == "bias+100":
        assert float(lg.max()) > 100.0
    else:
        assert span > 150.0
    want32, w32 = _run_oracle(ref, src, tgt, cand, G)
    ref64 = O.cpg().double()
    ref64.load_state_dict(ref.state_dict())
    want64, w64 = _run_oracle(ref64, src.double(), tgt.double(), cand.double(), G)
    assert torch.isfinite(want32).all() and torch.isfinite(want64).all()
    mine = _mine(ref, cuda)
    got, w = mine(src.to(cuda), tgt.to(cuda), cand.to(cuda), R_OF[G], S, return_weights=True)
    got, w = got.cpu(), w.cpu()
    err_o = float((want32.double() - want64).abs().max())
    err_g = float((got.double() - want64).abs().max())
    print(f"  max|fp32 oracle - fp64| {err_o:.2e}, max|gpu - fp64| {err_g:.2e} (bound {1e-5 + 4 * err_o:.2e}); "
          f"weights: oracle {float((w32.double() - w64).abs().max()):.2e}, gpu {float((w.double() - w64).abs().max()):.2e}")
    assert torch.isfinite(got).all() and torch.isfinite(w).all()
    assert err_g <= 1e-5 + 4 * err_o
    torch.testing.assert_close(w.sum(-1), torch.ones(w.shape[:2]), rtol=0, atol=1e-5)


def test_cpg_tiled_edges(cuda):
    from dvcp import ops
    G = 12
    C = G ** 3
    ref, src, tgt, cand, want, _ = _case(G)
    params = _mine(ref, cuda).packed_params()
    # no key point: empty outputs, no launch
    for B, K in ((0, 3), (2, 0)):
        v, w = ops.cpg(torch.zeros(B, K, 32, device=cuda), torch.zeros(B, K, 32, C, device=cuda),
                       torch.zeros(B, K, C, 3, device=cuda), G, params, want_weight=True)
        assert v.shape == (B, K, 3) and w.shape == (B, K, C)
        v = ops.cpg(torch.zeros(B, K, 32, device=cuda), torch.zeros(B, K, 32, C, device=cuda),
                    torch.zeros(B, K, C, 3, device=cuda), G, params, method="tiled")
        assert v.shape == (B, K, 3)
    # above the cap: a clear error that names the limit, on either method
    C33 = 33 ** 3
    for method in (None, "tiled"):
        with pytest.raises(ValueError, match="G <= 32"):
            ops.cpg(torch.zeros(1, 1, 32, device=cuda), torch.zeros(1, 1, 32, C33, device=cuda),
                    torch.zeros(1, 1, C33, 3, device=cuda), 33, params, method=method)
    with pytest.raises(RuntimeError, match="dvcp_cpg_tiled"):   # the LDS kernel points at the tiled entry
        ops.cpg(src.to(cuda), tgt.to(cuda), cand.to(cuda), G, params, method="lds")
    # with and without the weights output
    v1, w = ops.cpg(src.to(cuda), tgt.to(cuda), cand.to(cuda), G, params, want_weight=True)
    v0 = ops.cpg(src.to(cuda), tgt.to(cuda), cand.to(cuda), G, params)
    assert torch.equal(v0, v1)
    torch.testing.assert_close(v0.cpu(), want, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(w.sum(-1).cpu(), torch.ones(w.shape[:2]), rtol=0, atol=1e-5)
    assert (w >= 0).all()


def test_large_grid_training_raises(cuda, monkeypatch):
    """Large grids are inference-only: with autograd recording the forward raises before any
    launch (not dvcp_cpg_backward in the middle of loss.backward()), and dvcp_cpg_backward keeps
    its own cap."""
    import dvcp
    from dvcp import _lib, ops
    G = 13
    ref, src, tgt, cand, _, _ = _case(G)
    mine = dvcp.cpg().to(cuda)
    mine.load_state_dict(ref.state_dict())
    assert all(p.requires_grad for p in mine.parameters()) and torch.is_grad_enabled()
    log = []
    monkeypatch.setattr(_lib, "EVENT_LOG", log)
    with pytest.raises(NotImplementedError, match="inference-only"):
        mine(src.to(cuda), tgt.to(cuda), cand.to(cuda), R_OF[G], S)
    assert log == [], "an entry point was called before the guard"
    monkeypatch.setattr(_lib, "EVENT_LOG", None)
    with torch.no_grad():   # the same call without autograd runs
        assert mine(src.to(cuda), tgt.to(cuda), cand.to(cuda), R_OF[G], S).shape == (1, 3, 3)
    m = dvcp.DeepVCP(use_normal=False, K=32, r=1.5, s=S, fe_npoint=64).to(cuda)
    m.FE1.eval()
    m.FE1.requires_grad_(False)
    monkeypatch.setattr(_lib, "EVENT_LOG", log)
    x = torch.rand(1, 3, 256, device=cuda)
    with pytest.raises(NotImplementedError, match="inference-only"):
        m(x, x, torch.eye(3, dtype=torch.float64, device=cuda)[None], torch.zeros(1, 3))
    assert log == []
    monkeypatch.setattr(_lib, "EVENT_LOG", None)
    C = 12 ** 3
    with pytest.raises(RuntimeError, match="grid side"):
        ops.cpg_backward(torch.zeros(1, 1, 32, device=cuda), torch.zeros(1, 1, 32, C, device=cuda),
                         torch.zeros(1, 1, C, 3, device=cuda), 12, torch.zeros(ops.CPG_NPARAMS, device=cuda),
                         torch.zeros(1, 1, 3, device=cuda))


def test_e2e_large_grid_vs_oracle(cuda):
    """dvcp.DeepVCP at r = 1.5, s = 0.25 (G = 13, C = 2197) against oracle.DeepVCP, the stage-decoupled
    back half of test_gpu_e2e.py: the oracle's top-k fed in, then key points and candidates exact,
    the kNN of the first 4096 queries exact, target DFE, vcp and the pose within the usual bars."""
    import dvcp
    import oracle as O
    from dvcp.synthetic import condition_weights, make_pairs, randomize_bn
    B, N, K, r = 1, 2048, 32, 1.5
    src, tgt, R, t = make_pairs(B, N, seed=71)
    torch.manual_seed(0)
    ref = O.DeepVCP(use_normal=False, K=K, r=r, s=S, fe_npoint=512).eval()
    randomize_bn(ref)
    with torch.no_grad():
        _, calib = ref.FE1(src)
    condition_weights(ref, feats=calib)
    mine = dvcp.DeepVCP(use_normal=False, K=K, r=r, s=S, fe_npoint=512).eval()
    mine.load_state_dict(ref.state_dict())
    mine.to(cuda)
    starts = mine.draw_starts(B, N, N)
    with torch.no_grad(), O.fps_starts(list(starts)), O.tracing() as trace:
        kp_o, vcp_o = ref(src, tgt, R, torch.zeros(1, 3))
        _, R_o, t_o = O.deepVCP_loss(kp_o, vcp_o, R, t, 0.5)
    d = dict(trace)
    tr = {}
    with torch.no_grad():
        kp, vcp = mine(src.to(cuda), tgt.to(cuda), R.to(cuda), torch.zeros(1, 3), starts=starts,
                       keypoint_idx=d["topk_idx"], trace=tr)
        _, Rp, tp = dvcp.deepVCP_loss(kp, vcp, R.to(cuda), t.to(cuda), 0.5)
    C = 13 ** 3
    assert tr["cand"].shape == (B, K, C, 3)
    assert torch.equal(kp.cpu(), kp_o)
    assert torch.equal(tr["cand"].cpu(), d["candidates"])
    nq = 4096
    assert torch.equal(tr["knn_idx"][:, :nq].cpu().long(), d["knn_idx"][:, :nq]), "kNN indices differ from the oracle"
    assert torch.equal(tr["knn_dist"][:, :nq].cpu(), d["knn_dist"][:, :nq]), "kNN distances differ from the oracle"
    torch.testing.assert_close(tr["tgt_dfe"].cpu().reshape(d["tgt_dfe"].shape), d["tgt_dfe"], rtol=1e-4, atol=1e-5)
    print(f"e2e G=13: max|vcp err| {float((vcp.cpu() - vcp_o).abs().max()):.2e}, "
          f"max|dR| {float((Rp.cpu() - R_o).abs().max()):.2e}, max|dt| {float((tp.cpu() - t_o).abs().max()):.2e}")
    torch.testing.assert_close(vcp.cpu(), vcp_o, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(Rp.cpu(), R_o, rtol=0, atol=1e-4)
    torch.testing.assert_close(tp.cpu(), t_o, rtol=0, atol=1e-4)
