"""The large-grid CPG backward (dvcp_cpg_tiled_backward, 1 <= G <= 32; csrc/cpg_tiled_bwd.hip) against
torch autograd through the fp64 oracle (oracle/ref_r.py cpg), from the kernel up to dvcp.DeepVCP
with ``train_large_grid=True``.

Inputs follow test_gpu_train.py::test_cpg_backward_vs_oracle (seed 3, O.cpg().double(), target base
randn * 0.5 + 0.3 passed as the permuted view, random grad_vcp) and its bar: max |got - want| <=
2e-4 max |want| per tensor, conv3.bias floored at 1e-3 (its gradient vanishes analytically).  Grids
come from s = 0.25 (test_gpu_cpg_tiled.py's R_OF), so every int(2r/s + 1) is exact.  The backward's
blocks are per axis ceil(G / 8) blocks of ceil(G / blocks) cells: 12 = 6 + 6, 13 = 7 + 6 (odd C,
unequal blocks), 17 = 6 + 6 + 5, 23 = 8 + 8 + 7 (an interior block, a shorter last one), 32 = 4 x 8
(the cap); 11 forced = 6 + 5; up to 8 one block."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

S = 0.25
R_OF = {1: 0.0, 2: 0.125, 6: 0.625, 11: 1.25, 12: 1.375, 13: 1.5, 17: 2.0, 23: 2.75, 32: 3.875}
assert all(int((2 * r) / S + 1) == G for G, r in R_OF.items())
NAMES = [(c, p) for c in ("conv1", "conv2", "conv3") for p in ("weight", "bias")]
TOL = 2e-4


def _floor(name):
    return 1e-3 if name == ("conv3", "bias") else 1e-30


def _rel(got, want, floor=1e-30):
    """max |got - want| / max(max |want|, floor)"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max()) / max(float(want.abs().max()), floor) if want.numel() else 0.0


def _oracle_grads(ref, src, tgt_base, cand, gv, G):
    """Autograd through the oracle in the module's dtype: (vcp, d src, d tgt_base, {name: d param})."""
    dt = ref.conv1.weight.dtype
    ref.zero_grad()
    s_o = src.to(dt).clone().requires_grad_()
    t_o = tgt_base.to(dt).clone().requires_grad_()
    vcp = ref(s_o, t_o.permute(0, 1, 3, 2), cand.to(dt), R_OF[G], S)
    (vcp * gv.to(dt)).sum().backward()
    grads = {n: getattr(getattr(ref, n[0]), n[1]).grad.clone() for n in NAMES}
    return vcp.detach(), s_o.grad, t_o.grad, grads


@functools.lru_cache(maxsize=None)
def _case(G, B, K, bias=0.0):
    """One fp64 oracle run per case, shared by the tests (read-only)."""
    import oracle as O
    torch.manual_seed(3)
    ref = O.cpg().double()
    if bias:
        with torch.no_grad():
            ref.conv3.bias += bias
    C = G ** 3
    src = torch.randn(B, K, 1, 32, dtype=torch.float64)
    tgt_base = torch.randn(B, K, C, 32, dtype=torch.float64) * 0.5 + 0.3
    cand = torch.randn(B, K, C, 3, dtype=torch.float64)
    gv = torch.randn(B, K, 3, dtype=torch.float64)
    vcp, gs, gt, gp = _oracle_grads(ref, src, tgt_base, cand, gv, G)
    return dict(ref=ref, src=src, tgt_base=tgt_base, cand=cand, gv=gv, vcp=vcp, gsrc=gs, gtgt=gt, gp=gp)


def _mine(ref, cuda, **kw):
    import dvcp
    mine = dvcp.cpg(**kw).to(cuda)
    mine.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    return mine


def _check(what, errs, bound=None):
    """errs: {name: relative error}; all asserted at once, after printing every figure."""
    print(f"{what}: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for k, v in errs.items():
        b = bound[k] if isinstance(bound, dict) else (TOL if bound is None else bound)
        if k == "vcp" and bound is None:
            b = 1e-5
        assert v <= b, f"{what}: {k} relative error {v:.3e} above {b:.3e}"


def _module_errs(c, mine, cuda, G, tgt_leaf=None, tgt_view=None, tgt_grad=None, gv=None):
    """Forward + backward through the module; relative errors of every output against the case."""
    mine.zero_grad()
    s_g = c["src"].float().to(cuda).requires_grad_()
    if tgt_leaf is None:
        tgt_leaf = c["tgt_base"].float().to(cuda).requires_grad_()
        tgt_view = tgt_leaf.permute(0, 1, 3, 2)
        tgt_grad = lambda: tgt_leaf.grad   # noqa: E731
    vcp = mine(s_g, tgt_view, c["cand"].float().to(cuda), R_OF[G], S)
    vcp.backward(c["gv"].float().to(cuda) if gv is None else gv)
    errs = {"vcp": _rel(vcp, c["vcp"]), "d src": _rel(s_g.grad, c["gsrc"]), "d tgt": _rel(tgt_grad(), c["gtgt"])}
    for n in NAMES:
        errs[".".join(n)] = _rel(getattr(getattr(mine, n[0]), n[1]).grad, c["gp"][n], _floor(n))
    return errs


@pytest.mark.parametrize("G,B,K", [(12, 1, 2), (13, 2, 2), (17, 1, 2), (23, 1, 2), (32, 1, 1)])
def test_cpg_tiled_backward_vs_oracle(cuda, G, B, K):
    """dvcp.cpg(train_large_grid=True) on grids above 11^3: vcp (1e-5 of max), d src, d tgt and the
    six parameter gradients at test_cpg_backward_vs_oracle's bar."""
    from dvcp import ops
    assert ops.cpg_method(G) == "tiled"
    c = _case(G, B, K)
    mine = _mine(c["ref"], cuda, train_large_grid=True)
    _check(f"cpg tiled backward G={G}", _module_errs(c, mine, cuda, G))


def _split(gp):
    sizes = [16 * 32 * 27, 16, 4 * 16 * 27, 4, 4 * 27, 1]
    return dict(zip(NAMES, torch.split(gp, sizes)))


def _ops_errs(out, c):
    gsrc, gtgt, gp = out
    errs = {"d src": _rel(gsrc, c["gsrc"].reshape(gsrc.shape)), "d tgt": _rel(gtgt, c["gtgt"].permute(0, 1, 3, 2))}
    for n, g in _split(gp).items():
        errs[".".join(n)] = _rel(g, c["gp"][n].reshape(-1), _floor(n))
    return errs


@pytest.mark.parametrize("G", [1, 2, 6, 11])
def test_cpg_tiled_backward_small_grids_match_lds_backward(cuda, G):
    """The tiled backward at the one-workgroup backward's grids: both against each other (2e-4 of
    each output's max) and against the oracle.  G = 1 is below dvcp_cpg_backward's range: tiled
    against the oracle only."""
    from dvcp import ops
    B, K = 2, 3
    c = _case(G, B, K)
    params = _mine(c["ref"], cuda).packed_params().detach()
    args = (c["src"].float().to(cuda).view(B, K, 32), c["tgt_base"].float().to(cuda).permute(0, 1, 3, 2),
            c["cand"].float().to(cuda), G, params, c["gv"].float().to(cuda))
    til = ops.cpg_tiled_backward(*args)
    _check(f"tiled backward G={G} vs oracle", _ops_errs(til, c))
    if G == 1:
        return
    lds = ops.cpg_backward(*args)
    _check(f"lds backward G={G} vs oracle", _ops_errs(lds, c))
    errs = {"d src": _rel(til[0], lds[0]), "d tgt": _rel(til[1], lds[1])}
    for (n, a), b in zip(_split(til[2]).items(), _split(lds[2]).values()):
        errs[".".join(n)] = _rel(a, b, _floor(n))
    _check(f"tiled vs lds backward G={G}", errs)


def test_cpg_tiled_backward_chunks_and_determinism(cuda):
    """G = 12, five key points, a workspace for two: three chunks, the last one short.  Every
    output bit-equal to the default workspace's (one chunk) and to a second identical call."""
    import dvcp
    from dvcp import ops
    G, B, K = 12, 1, 5
    C = G ** 3
    g = torch.Generator().manual_seed(17)
    src = torch.randn(B, K, 32, generator=g).to(cuda)
    tgt = (torch.randn(B, K, C, 32, generator=g) * 0.5 + 0.3).to(cuda).permute(0, 1, 3, 2)
    cand = torch.randn(B, K, C, 3, generator=g).to(cuda)
    gv = torch.randn(B, K, 3, generator=g).to(cuda)
    torch.manual_seed(3)
    params = dvcp.cpg().to(cuda).packed_params().detach()
    size = dvcp.load_library().dvcp_cpg_tiled_backward_workspace_bytes
    partials = lambda P: (P * ops.CPG_NPARAMS + 3) // 4 * 16   # noqa: E731
    per = int(size(1, G)) - partials(1)
    assert int(size(K, G)) == partials(K) + K * per    # the default: all five in one chunk
    one = ops.cpg_tiled_backward(src, tgt, cand, G, params, gv)
    two = ops.cpg_tiled_backward(src, tgt, cand, G, params, gv, ws_bytes=partials(K) + 2 * per)
    again = ops.cpg_tiled_backward(src, tgt, cand, G, params, gv, ws_bytes=partials(K) + 2 * per)
    single = ops.cpg_tiled_backward(src, tgt, cand, G, params, gv, ws_bytes=partials(K) + per)
    for name, a, b, c3, d in zip(("d src", "d tgt", "d params"), one, two, again, single):
        assert torch.isfinite(a).all() and float(a.abs().max()) > 0, name
        assert torch.equal(a, b), f"{name}: three chunks differ from one"
        assert torch.equal(b, c3), f"{name}: two identical calls differ"
        assert torch.equal(a, d), f"{name}: five chunks differ from one"
    with pytest.raises(RuntimeError, match="workspace"):
        ops.cpg_tiled_backward(src, tgt, cand, G, params, gv, ws_bytes=partials(K) + per - 16)


def test_cpg_tiled_backward_layouts(cuda):
    """G = 13: the target as the permuted view of (B, K, C, 32), as a contiguous (B, K, 32, C)
    tensor and as a batch slice whose stride(0) != K * stride(1); grad_vcp a non-contiguous slice."""
    G, B, K = 13, 2, 2
    C = G ** 3
    c = _case(G, B, K)
    mine = _mine(c["ref"], cuda, train_large_grid=True)
    gwide = torch.zeros(B, K, 4, device=cuda)
    gwide[..., :3] = c["gv"].float().to(cuda)
    gv = gwide[..., :3]
    assert not gv.is_contiguous()
    base = c["tgt_base"].float().to(cuda)

    view_leaf = base.clone().requires_grad_()
    view = view_leaf.permute(0, 1, 3, 2)
    assert view.stride(2) == 1 and view.stride(3) == 32
    _check("permuted view", _module_errs(c, mine, cuda, G, view_leaf, view, lambda: view_leaf.grad, gv))

    dense = base.permute(0, 1, 3, 2).contiguous().requires_grad_()
    assert dense.stride(2) == C and dense.stride(3) == 1
    _check("contiguous", _module_errs(c, mine, cuda, G, dense, dense, lambda: dense.grad.permute(0, 1, 3, 2), gv))

    wide = torch.zeros(B, K + 1, 32, C, device=cuda)
    wide[:, :K] = base.permute(0, 1, 3, 2)
    wide.requires_grad_()
    sliced = wide[:, :K]
    assert sliced.stride(0) != K * sliced.stride(1)
    errs = _module_errs(c, mine, cuda, G, wide, sliced, lambda: wide.grad[:, :K].permute(0, 1, 3, 2), gv)
    _check("batch slice", errs)
    assert float(wide.grad[:, K:].abs().max()) == 0.0


def test_cpg_tiled_backward_softmax_range(cuda):
    """G = 12 with conv3.bias + 100: every logit above exp's fp32 overflow unless the key point's
    global maximum is subtracted across blocks.  All gradients finite and within 2e-4 + 4 e32 of the
    fp64 oracle, e32 the fp32 oracle's own relative error on that tensor in this run
    (test_cpg_tiled_softmax_range's form of bound: the GPU's error is of the fp32 oracle's kind)."""
    import oracle as O
    G, B, K = 12, 1, 2
    c = _case(G, B, K, 100.0)
    ref32 = O.cpg()
    ref32.load_state_dict({k: v.float() for k, v in c["ref"].state_dict().items()})
    assert float(ref32.conv3.bias.detach()) > 99.0
    v32, gs32, gt32, gp32 = _oracle_grads(ref32, c["src"], c["tgt_base"], c["cand"], c["gv"], G)
    e32 = {"vcp": _rel(v32, c["vcp"]), "d src": _rel(gs32, c["gsrc"]), "d tgt": _rel(gt32, c["gtgt"])}
    for n in NAMES:
        e32[".".join(n)] = _rel(gp32[n], c["gp"][n], _floor(n))
    print("fp32 oracle vs fp64: " + ", ".join(f"{k} {v:.1e}" for k, v in e32.items()))
    mine = _mine(c["ref"], cuda, train_large_grid=True)
    s_g = c["src"].float().to(cuda).requires_grad_()
    t_g = c["tgt_base"].float().to(cuda).requires_grad_()
    vcp = mine(s_g, t_g.permute(0, 1, 3, 2), c["cand"].float().to(cuda), R_OF[G], S)
    (vcp * c["gv"].float().to(cuda)).sum().backward()
    for t in [vcp, s_g.grad, t_g.grad] + [p.grad for p in mine.parameters()]:
        assert torch.isfinite(t).all()
    errs = {"vcp": _rel(vcp, c["vcp"]), "d src": _rel(s_g.grad, c["gsrc"]), "d tgt": _rel(t_g.grad, c["gtgt"])}
    for n in NAMES:
        errs[".".join(n)] = _rel(getattr(getattr(mine, n[0]), n[1]).grad, c["gp"][n], _floor(n))
    _check("bias + 100", errs, {k: TOL + 4 * e32[k] for k in errs})


def test_cpg_tiled_backward_edges(cuda):
    from dvcp import ops
    G = 12
    C = G ** 3
    c = _case(G, 1, 2)
    params = _mine(c["ref"], cuda).packed_params().detach()
    # no key point: empty gradients, zero parameter gradients, no error
    for B, K in ((0, 3), (2, 0)):
        gs, gt, gp = ops.cpg_tiled_backward(torch.zeros(B, K, 32, device=cuda), torch.zeros(B, K, 32, C, device=cuda),
                                            torch.zeros(B, K, C, 3, device=cuda), G, params,
                                            torch.zeros(B, K, 3, device=cuda))
        assert gs.shape == (B, K, 32) and gt.shape == (B, K, 32, C)
        assert gp.shape == (ops.CPG_NPARAMS,) and float(gp.abs().max()) == 0.0
    C33 = 33 ** 3
    with pytest.raises(ValueError, match="G <= 32"):
        ops.cpg_tiled_backward(torch.zeros(1, 1, 32, device=cuda), torch.zeros(1, 1, 32, C33, device=cuda),
                               torch.zeros(1, 1, C33, 3, device=cuda), 33, params, torch.zeros(1, 1, 3, device=cuda))
    src = c["src"].float().to(cuda)
    tgt = c["tgt_base"].float().to(cuda).permute(0, 1, 3, 2)
    cand = c["cand"].float().to(cuda)
    gv = c["gv"].float().to(cuda)
    # inputs that need no gradient, trainable weights: only the parameter gradients are filled
    mine = _mine(c["ref"], cuda, train_large_grid=True)
    (mine(src, tgt, cand, R_OF[G], S) * gv).sum().backward()
    assert src.grad is None and tgt.grad is None
    for n in NAMES:
        assert _rel(getattr(getattr(mine, n[0]), n[1]).grad, c["gp"][n], _floor(n)) <= TOL, n
    # frozen weights, src needs a gradient: only d src
    mine = _mine(c["ref"], cuda, train_large_grid=True).requires_grad_(False)
    s_g = src.clone().requires_grad_()
    (mine(s_g, tgt, cand, R_OF[G], S) * gv).sum().backward()
    assert all(p.grad is None for p in mine.parameters()) and tgt.grad is None
    assert _rel(s_g.grad, c["gsrc"]) <= TOL
    # without the opt-in the same call is refused, as before
    with pytest.raises(NotImplementedError, match="inference-only"):
        _mine(c["ref"], cuda)(s_g, tgt, cand, R_OF[G], S)


def test_head_train_step_large_grid_vs_oracle(cuda):
    """test_gpu_train.py::test_head_train_step_vs_oracle at r = 1.5, s = 0.25 (G = 13, C = 2197) with
    train_large_grid=True: the frozen-extractor training step end to end.  K stays 32 (the oracle's
    key-point grouping takes 32 neighbours)."""
    import oracle as O
    import dvcp
    from dvcp.synthetic import condition_weights, make_pairs, randomize_bn
    src, tgt, R_gt, t_gt = make_pairs(1, 1024, seed=91)
    torch.manual_seed(0)
    ref = O.DeepVCP(use_normal=False, K=32, r=1.5, s=S, fe_npoint=512)
    randomize_bn(ref)
    ref.FE1.eval()
    with torch.no_grad():
        _, calib = ref.FE1(src)
    condition_weights(ref, feats=calib)
    ref.FE1.requires_grad_(False)
    mine = dvcp.DeepVCP(use_normal=False, K=32, r=1.5, s=S, fe_npoint=512, train_large_grid=True)
    mine.load_state_dict(ref.state_dict())
    mine.to(cuda)
    mine.FE1.eval()
    mine.FE1.requires_grad_(False)

    torch.manual_seed(1)
    with O.tracing() as trace:
        kp_o, vcp_o = ref(src, tgt, R_gt, torch.zeros(1, 3))
    loss_o, _, _ = O.deepVCP_loss(kp_o, vcp_o, R_gt, t_gt, 0.5)
    loss_o.backward()
    top = dict(trace)["topk_idx"]

    torch.manual_seed(1)
    kp, vcp = mine(src.to(cuda), tgt.to(cuda), R_gt.to(cuda), torch.zeros(1, 3), keypoint_idx=top)
    assert vcp.requires_grad and not kp.requires_grad
    loss, _, _ = dvcp.deepVCP_loss(kp, vcp, R_gt.to(cuda), t_gt.to(cuda), 0.5)
    loss.backward()
    print(f"loss {float(loss.detach()):.6f} (oracle {float(loss_o.detach()):.6f})")
    errs, scale = {}, {}
    for mod in ("DFE.fc1", "DFE.fc2", "DFE.fc3", "cpg.conv1", "cpg.conv2", "cpg.conv3"):
        a, b = mod.split(".")
        for p in ("weight", "bias"):
            got = getattr(getattr(getattr(mine, a), b), p).grad
            want = getattr(getattr(getattr(ref, a), b), p).grad
            errs[f"{mod}.{p}"] = _rel(got, want, 1e-3 if (mod, p) == ("cpg.conv3", "bias") else 1e-30)
            scale[f"{mod}.{p}"] = float(want.abs().max())
    print("oracle gradient scales:", {k: f"{v:.1e}" for k, v in scale.items()})
    torch.testing.assert_close(loss.detach().cpu(), loss_o.detach(), rtol=1e-4, atol=1e-6)
    _check("head training step G=13", errs, 1e-3)
    assert scale["cpg.conv1.weight"] > 1e-5    # the comparison is not vacuous
    assert all(p.grad is None for p in mine.FE1.parameters())
    opt = torch.optim.Adam([p for p in mine.parameters() if p.requires_grad], lr=1e-3)
    before = mine.cpg.conv1.weight.detach().clone()
    opt.step()
    assert not torch.equal(before, mine.cpg.conv1.weight.detach())


def test_training_mode_large_grid_runs(cuda):
    """test_training_mode_fe_batch_stats_runs at G = 13: the whole model in training mode, forward,
    loss and backward; every parameter gets a finite gradient and the running statistics move."""
    import dvcp
    torch.manual_seed(5)
    m = dvcp.DeepVCP(use_normal=False, K=32, r=1.5, s=S, fe_npoint=64, train_large_grid=True).to(cuda)
    x = torch.rand(1, 3, 128, device=cuda)
    rm0 = m.FE1.sa1.mlp_bns[0].running_mean.clone()
    eye = torch.eye(3, dtype=torch.float64, device=cuda)[None]
    kp, vcp = m(x, x, eye, torch.zeros(1, 3))
    loss, _, _ = dvcp.deepVCP_loss(kp, vcp, eye, torch.zeros(1, 3, 1, dtype=torch.float64, device=cuda), 0.5)
    loss.backward()
    assert torch.isfinite(loss)
    # every parameter the step reaches: the ones the same step reaches on the default grid (the
    # weighting layer feeds the non-differentiable top-k only, there as here)
    torch.manual_seed(5)
    small = dvcp.DeepVCP(use_normal=False, K=32, fe_npoint=64).to(cuda)
    kp0, vcp0 = small(x, x, eye, torch.zeros(1, 3))
    dvcp.deepVCP_loss(kp0, vcp0, eye, torch.zeros(1, 3, 1, dtype=torch.float64, device=cuda), 0.5)[0].backward()
    reached = {n for n, p in small.named_parameters() if p.grad is not None}
    assert {n for n, p in m.named_parameters() if p.grad is not None} == reached
    assert all(n in reached for n, _ in m.named_parameters() if n.split(".")[0] in ("FE1", "DFE", "cpg"))
    for name, p in m.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all(), name
    assert float(m.cpg.conv1.weight.grad.abs().max()) > 0
    assert int(m.FE1.sa1.mlp_bns[0].num_batches_tracked) == 2   # src and tgt: two FE1 calls
    assert not torch.equal(rm0, m.FE1.sa1.mlp_bns[0].running_mean)
