"""Paper mode, training of the stage heads (dvcp.paper with autograd): the 1-D CPG backward
(dvcp_cpg1d_backward) and the weighting layer's backward (dvcp_weighting_backward; both
csrc/paper_bwd.hip) against torch autograd through the checker's modules (oracle/paper.py) in fp64,
then the modules, then DeepVCPPaper(train_heads=True) against the checker's own training step.

Bars.  1-D CPG: test_gpu_train.py::test_cpg_backward_vs_oracle's -- vcp within 1e-5, d src, d tgt
and the six parameter gradients within 2e-4 of each tensor's maximum, conv3.bias floored at 1e-3
(softmax is shift invariant: its true gradient is zero).  Weighting layer: the head kernels' 1e-4 of
each tensor's maximum.  Head training step: test_head_train_step_vs_oracle's -- loss rtol 1e-4,
parameter gradients 1e-3 of each tensor's maximum, floored at 1e-3 where the true gradient is zero:
both stages' cpg.conv3.bias (each CPG ends in a softmax; the 3-D one is the tensor that test floors)
and the DFE's three biases (a DFE bias adds the same constant to the source and the target
embedding -- linear layers, then a max over the neighbours -- and the CPG reads only their
difference; the checker's own values there are 1e-9, rounding of sums whose terms are 1e-2).

The 1-D backward runs min(P, 256) workgroups that walk key points p, p + 256, ...: no workgroup is
ever idle, so the cases cover one key point per workgroup (P <= 256), one and two (P = 257), and two
and three (P = 600); P = 0 launches nothing."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CONVS = [(c, p) for c in ("conv1", "conv2", "conv3") for p in ("weight", "bias")]
TOL = 2e-4
# Gz -> (B, K)
CPG1D_CASES = {1: (1, 1), 2: (2, 3), 3: (1, 7), 9: (2, 24), 17: (2, 300), 64: (1, 257)}


def _floor(name):
    return 1e-3 if name == ("conv3", "bias") else 1e-30


def _rel(got, want, floor=1e-30):
    """max |got - want| / max(max |want|, floor)"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((got - want).abs().max()) / max(float(want.abs().max()), floor) if want.numel() else 0.0


def _check(what, errs, bound):
    """errs: {name: relative error}; bound: one number or {name: bound}.  Every figure is printed
    before any is asserted."""
    print(f"{what}: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for k, v in errs.items():
        b = bound[k] if isinstance(bound, dict) else bound
        assert v <= b, f"{what}: {k} relative error {v:.3e} above {b:.3e}"


def _randomize_bn(model, seed=3):
    """tests/test_gpu_paper.py's recipe."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                n = m.num_features
                m.weight.copy_(torch.rand(n, generator=g) + 0.5)
                m.bias.copy_(torch.rand(n, generator=g) * 0.2 - 0.1)
                m.running_mean.copy_(torch.rand(n, generator=g) * 0.2 - 0.1)
                m.running_var.copy_(torch.rand(n, generator=g) + 0.5)


# ------------------------------------------------------------------------------------ 1-D CPG
def _cpg1d_oracle(ref, src, tgt, cand, gv):
    """Autograd through the checker in the module's dtype: (vcp, d src, d tgt, {name: d param})."""
    dt = ref.conv1.weight.dtype
    ref.zero_grad()
    s_o = src.to(dt).clone().requires_grad_()
    t_o = tgt.to(dt).clone().requires_grad_()
    vcp = ref(s_o, t_o, cand.to(dt))
    (vcp * gv.to(dt)).sum().backward()
    grads = {n: getattr(getattr(ref, n[0]), n[1]).grad.clone() for n in CONVS}
    return vcp.detach(), s_o.grad, t_o.grad, grads


@functools.lru_cache(maxsize=None)
def _cpg1d_case(Gz, B, K, variant=""):
    """One fp64 checker run per case, shared by the tests (read-only).  Inputs as
    test_gpu_paper.py::test_cpg1d_vs_oracle (fp32 randn from generator 63, the module from seed 7)."""
    from oracle import paper as OP
    g = torch.Generator().manual_seed(63 + Gz)
    torch.manual_seed(7)
    ref = OP.CPG1D().double()
    with torch.no_grad():
        if variant == "bias+100":
            ref.conv3.bias += 100.0
        elif variant == "weight*50":
            ref.conv3.weight *= 50.0
    src = torch.randn(B, K, 32, generator=g)
    tgt = torch.randn(B, K, Gz, 32, generator=g)
    cand = torch.randn(B, K, Gz, 3, generator=g)
    gv = torch.randn(B, K, 3, generator=g)
    vcp, gs, gt, gp = _cpg1d_oracle(ref, src, tgt, cand, gv)
    return dict(ref=ref, src=src, tgt=tgt, cand=cand, gv=gv, vcp=vcp, gsrc=gs, gtgt=gt, gp=gp)


def _cpg1d_mine(ref, cuda):
    import dvcp
    mine = dvcp.paper.CPG1D().eval()
    mine.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    return mine.to(cuda)


def _cpg1d_module_errs(c, mine, cuda):
    mine.zero_grad()
    s_g = c["src"].to(cuda).requires_grad_()
    t_g = c["tgt"].to(cuda).requires_grad_()
    vcp = mine(s_g, t_g, c["cand"].to(cuda))
    assert vcp.requires_grad
    (vcp * c["gv"].to(cuda)).sum().backward()
    outs = [vcp, s_g.grad, t_g.grad] + [p.grad for p in mine.parameters()]
    assert all(torch.isfinite(t).all() for t in outs)
    errs = {"vcp": _rel(vcp, c["vcp"]), "d src": _rel(s_g.grad, c["gsrc"]), "d tgt": _rel(t_g.grad, c["gtgt"])}
    for n in CONVS:
        errs[".".join(n)] = _rel(getattr(getattr(mine, n[0]), n[1]).grad, c["gp"][n], _floor(n))
    return errs


def _cpg1d_bounds():
    return {"vcp": 1e-5, "d src": TOL, "d tgt": TOL, **{".".join(n): TOL for n in CONVS}}


@pytest.mark.parametrize("Gz", sorted(CPG1D_CASES))
def test_cpg1d_backward_vs_oracle(cuda, Gz):
    """dvcp.paper.CPG1D with autograd on against the fp64 checker.  Gz = 1: the softmax of one logit
    is constant, every gradient is exactly zero on both sides (and finite).  Gz = 2, 3: the line is
    shorter than or as long as the kernel.  Gz = 64: the cap, no padding lane.  Gz = 17 runs 600 key
    points (workgroups with two and three), Gz = 64 257 (one and two)."""
    B, K = CPG1D_CASES[Gz]
    c = _cpg1d_case(Gz, B, K)
    errs = _cpg1d_module_errs(c, _cpg1d_mine(c["ref"], cuda), cuda)
    _check(f"cpg1d backward Gz={Gz} P={B * K}", errs, _cpg1d_bounds())
    if Gz == 1:
        assert all(float(v.abs().max()) == 0.0 for v in c["gp"].values()) and float(c["gtgt"].abs().max()) == 0.0


@pytest.mark.parametrize("variant", ["bias+100", "weight*50"])
def test_cpg1d_backward_softmax_range(cuda, variant):
    """conv3.bias + 100 (every logit above exp's fp32 overflow unless the row maximum is subtracted)
    and conv3.weight * 50 (a wide logit range): finite, and within 2e-4 + 4 e32 of the fp64 checker,
    e32 the fp32 checker's own relative error on that tensor (test_cpg_tiled_backward_softmax_range's
    bound: the GPU's error is of the fp32 checker's kind)."""
    from oracle import paper as OP
    Gz, B, K = 17, 2, 5
    c = _cpg1d_case(Gz, B, K, variant)
    ref32 = OP.CPG1D()
    ref32.load_state_dict({k: v.float() for k, v in c["ref"].state_dict().items()})
    v32, gs32, gt32, gp32 = _cpg1d_oracle(ref32, c["src"], c["tgt"], c["cand"], c["gv"])
    e32 = {"vcp": _rel(v32, c["vcp"]), "d src": _rel(gs32, c["gsrc"]), "d tgt": _rel(gt32, c["gtgt"])}
    for n in CONVS:
        e32[".".join(n)] = _rel(gp32[n], c["gp"][n], _floor(n))
    print("fp32 checker vs fp64: " + ", ".join(f"{k} {v:.1e}" for k, v in e32.items()))
    errs = _cpg1d_module_errs(c, _cpg1d_mine(c["ref"], cuda), cuda)   # asserts finiteness
    _check(f"cpg1d backward {variant}", errs, {k: TOL + 4 * e32[k] for k in errs})


def test_cpg1d_backward_edges(cuda):
    from dvcp import ops
    Gz, (B, K) = 9, CPG1D_CASES[9]
    c = _cpg1d_case(Gz, B, K)
    mine = _cpg1d_mine(c["ref"], cuda)
    params = mine.packed_params()
    z = lambda *s: torch.zeros(*s, device=cuda)   # noqa: E731
    # no key point: empty input gradients, zero parameter gradients
    for b, k in ((0, 3), (2, 0)):
        gs, gt, gp = ops.cpg1d_backward(z(b, k, 32), z(b, k, Gz, 32), z(b, k, Gz, 3), params, z(b, k, 3))
        assert gs.shape == (b, k, 32) and gt.shape == (b, k, Gz, 32)
        assert gp.shape == (1761,) and float(gp.abs().max()) == 0.0
    with pytest.raises(RuntimeError, match=r"dvcp_cpg1d_backward: Gz=65 unsupported \(1\.\.64\)"):
        ops.cpg1d_backward(z(1, 1, 32), z(1, 1, 65, 32), z(1, 1, 65, 3), params, z(1, 1, 3))
    src, tgt, cand, gv = (c[k].to(cuda) for k in ("src", "tgt", "cand", "gv"))
    # two identical calls: identical bits in every output
    one = ops.cpg1d_backward(src, tgt, cand, params, gv)
    two = ops.cpg1d_backward(src, tgt, cand, params, gv)
    assert all(torch.equal(a, b) for a, b in zip(one, two))
    # null grad_src / grad_tgt: the parameter gradients are the same bits
    for ws, wt in ((False, False), (True, False), (False, True)):
        gs, gt, gp = ops.cpg1d_backward(src, tgt, cand, params, gv, want_src=ws, want_tgt=wt)
        assert (gs is None) == (not ws) and (gt is None) == (not wt)
        assert torch.equal(gp, one[2])
        assert gs is None or torch.equal(gs, one[0])
        assert gt is None or torch.equal(gt, one[1])
    # needs_input_grad through the module: inputs that need none, trainable weights
    (mine(src, tgt, cand) * gv).sum().backward()
    assert src.grad is None and tgt.grad is None
    for n in CONVS:
        assert _rel(getattr(getattr(mine, n[0]), n[1]).grad, c["gp"][n], _floor(n)) <= TOL, n
    # frozen weights, src needs a gradient: only d src
    frozen = _cpg1d_mine(c["ref"], cuda).requires_grad_(False)
    s_g = src.clone().requires_grad_()
    out = frozen(s_g, tgt, cand)
    (out * gv).sum().backward()
    assert all(p.grad is None for p in frozen.parameters()) and tgt.grad is None
    assert _rel(s_g.grad, c["gsrc"]) <= TOL
    # the autograd path runs the inference path's kernel: the same bits
    with torch.no_grad():
        plain = mine(src, tgt, cand)
    assert not plain.requires_grad and torch.equal(out.detach(), plain)
    assert torch.equal(mine(src, tgt, cand).detach(), plain)


# ----------------------------------------------------------------------------- weighting layer
WL_NAMES = [(m, p) for m in ("fc1", "bn1", "fc2", "bn2", "fc3") for p in ("weight", "bias")]


@functools.lru_cache(maxsize=None)
def _wl_case(P, shift=0.0):
    """fp64 checker run (randomised BN statistics and affine), shared and read-only.  Asserts that
    no ReLU pre-activation of the case lies within 1e-6 of zero (a unit that close to its kink may
    be masked differently in fp32)."""
    from oracle import paper as OP
    torch.manual_seed(11)
    ref = OP.PaperWeighting().eval()
    _randomize_bn(ref, seed=12)
    ref = ref.double()
    with torch.no_grad():
        ref.fc3.bias += shift
    g = torch.Generator().manual_seed(100 + P)
    feat = torch.randn(1, P, 32, generator=g)
    gs = torch.randn(1, P, generator=g)
    with torch.no_grad():
        pre1 = ref.bn1(ref.fc1(feat.double().reshape(P, 32)))
        pre2 = ref.bn2(ref.fc2(torch.relu(pre1)))
    margin = min(float(pre1.abs().min()), float(pre2.abs().min()))
    assert margin > 1e-6, f"P={P}: a ReLU pre-activation within {margin:.1e} of zero; choose another seed"
    f_o = feat.double().clone().requires_grad_()
    score = ref(f_o)
    (score * gs.double()).sum().backward()
    gp = {n: getattr(getattr(ref, n[0]), n[1]).grad.clone() for n in WL_NAMES}
    return dict(ref=ref, feat=feat, gs=gs, score=score.detach(), gfeat=f_o.grad, gp=gp, margin=margin)


def _wl_mine(ref, cuda):
    import dvcp
    mine = dvcp.paper.PaperWeighting().eval()
    mine.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in ref.state_dict().items()})
    return mine.to(cuda)


def _wl_errs(c, mine, cuda):
    mine.zero_grad()
    f_g = c["feat"].to(cuda).requires_grad_()
    score = mine(f_g)
    assert score.requires_grad
    (score * c["gs"].to(cuda)).sum().backward()
    assert all(torch.isfinite(t).all() for t in [score, f_g.grad] + [p.grad for p in mine.parameters()])
    errs = {"score": _rel(score, c["score"]), "d feat": _rel(f_g.grad, c["gfeat"])}
    for n in WL_NAMES:
        errs[".".join(n)] = _rel(getattr(getattr(mine, n[0]), n[1]).grad, c["gp"][n])
    return errs, score.detach()


@pytest.mark.parametrize("P", [1, 63, 64, 65, 1000])
def test_weighting_backward_vs_oracle(cuda, P):
    """dvcp.paper.PaperWeighting with autograd on against the fp64 checker: d feat and the gradients
    of fc1-3 and bn1-2 weight / bias within 1e-4 of each tensor's maximum (the BN fold is
    differentiated by torch).  P = 63, 64, 65: around the 64-row tile; 1000: several tiles per launch,
    the last one partial."""
    c = _wl_case(P)
    mine = _wl_mine(c["ref"], cuda)
    errs, score = _wl_errs(c, mine, cuda)
    print(f"smallest |ReLU pre-activation| {c['margin']:.1e}")
    _check(f"weighting backward P={P}", errs, 1e-4)
    with torch.no_grad():
        plain = mine(c["feat"].to(cuda))
    assert not plain.requires_grad and torch.equal(score, plain)   # the same kernel: the same bits
    assert all(p.grad is None for p in (mine.bn1.running_mean, mine.bn1.running_var))


@pytest.mark.parametrize("shift", [25.0, -30.0])
def test_weighting_backward_softplus_branches(cuda, shift):
    """fc3.bias + 25: every row on the forward's v > 20 branch (derivative 1); fc3.bias - 30: the
    logistic's far tail.  Finite and within the same bar."""
    c = _wl_case(65, shift)
    with torch.no_grad():
        v = torch.log(torch.expm1(c["score"]))
    assert bool((v > 20).all()) if shift > 0 else bool((c["score"] < 1e-11).all())
    errs, _ = _wl_errs(c, _wl_mine(c["ref"], cuda), cuda)
    _check(f"weighting backward fc3.bias {shift:+.0f}", errs, 1e-4)


def test_weighting_backward_edges(cuda):
    from dvcp import ops
    c = _wl_case(65)
    mine = _wl_mine(c["ref"], cuda)
    params = mine.packed_params()
    assert params.shape == (ops.WEIGHTING_NPARAMS,) and torch.equal(params, mine.folded_params().detach())
    # P = 0
    gp, gf = ops.weighting_backward(torch.zeros(0, 32, device=cuda), params, torch.zeros(0, device=cuda))
    assert gf.shape == (0, 32) and gp.shape == (673,) and float(gp.abs().max()) == 0.0
    # two calls, and grad_feat null: identical bits
    feat = c["feat"].to(cuda).reshape(65, 32)
    gs = c["gs"].to(cuda).reshape(65)
    one = ops.weighting_backward(feat, params, gs)
    two = ops.weighting_backward(feat, params, gs)
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
    gp, gf = ops.weighting_backward(feat, params, gs, want_feat=False)
    assert gf is None and torch.equal(gp, one[0])
    # an input that needs no gradient: the parameters still get theirs
    x = c["feat"].to(cuda)
    (mine(x) * c["gs"].to(cuda)).sum().backward()
    assert x.grad is None
    for n in WL_NAMES:
        assert _rel(getattr(getattr(mine, n[0]), n[1]).grad, c["gp"][n]) <= 1e-4, n
    # frozen layer, features that need a gradient
    frozen = _wl_mine(c["ref"], cuda).requires_grad_(False)
    x = c["feat"].to(cuda).requires_grad_()
    (frozen(x) * c["gs"].to(cuda)).sum().backward()
    assert all(p.grad is None for p in frozen.parameters()) and _rel(x.grad, c["gfeat"]) <= 1e-4


# ------------------------------------------------------------------------------------ modules
def test_modules_carry_gradient(cuda):
    """CPG1D().eval() and PaperWeighting().eval() called with autograd on: the outputs require a
    gradient and backward() fills every parameter's .grad with finite values that are not all zero."""
    import dvcp
    torch.manual_seed(21)
    cpg = dvcp.paper.CPG1D().eval().to(cuda)
    wl = dvcp.paper.PaperWeighting().eval().to(cuda)
    _randomize_bn(wl)
    B, K, Gz = 2, 5, 9
    vcp = cpg(torch.randn(B, K, 32, device=cuda), torch.randn(B, K, Gz, 32, device=cuda),
              torch.randn(B, K, Gz, 3, device=cuda))
    score = wl(torch.randn(B, 40, 32, device=cuda))
    assert vcp.requires_grad and score.requires_grad
    (vcp * torch.randn(B, K, 3, device=cuda)).sum().backward()
    (score * torch.randn(B, 40, device=cuda)).sum().backward()
    for mod in (cpg, wl):
        for name, p in mod.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
            if name != "conv3.bias":   # zero by the softmax's shift invariance, up to rounding
                assert float(p.grad.abs().max()) > 0.0, name
    for mod in (cpg, wl):   # training mode is still refused
        with pytest.raises(NotImplementedError, match="training mode"):
            mod.train()(*([torch.zeros(1, 1, 32, device=cuda)] * (3 if mod is cpg else 1)))


# ------------------------------------------------------------------------- the whole network
CFG = dict(K=8, r=0.4, s=0.4, s_z=0.25, d=1.0, npoints=(128, 32, 8))   # a 3^3 grid and a 4-point z line


def _checker_forward(ref, src, tgt, R_init, t_init):
    """oracle/paper.py DeepVCPPaper.forward, statement for statement, for a forward that records
    autograd: the checker's numpy pose solve takes ``vcp`` and ``w`` detached (Tensor.numpy() refuses
    a tensor that requires grad); nothing else differs.  The caller asserts that its values are the
    checker's own forward's."""
    from oracle import paper as OP
    from oracle import ref_r as R_
    B = src.shape[0]
    f_src, f_tgt = ref.FE(src), ref.FE(tgt)
    xs, xt = src[:, :3].permute(0, 2, 1), tgt[:, :3].permute(0, 2, 1)
    Rc, tc = R_init.double().expand(B, 3, 3), t_init.double().reshape(-1, 3).expand(B, 3)
    out = []
    for st in ref.stages:
        score = st.WL(f_src)
        w, top = torch.topk(score, ref.K, dim=1)
        kp = R_.index_points(xs, top)
        rows = OP.group_rows(kp, xs, f_src, ref.d, ref.ns)
        src_dfe = st.DFE(rows, src=True)
        moved = torch.einsum("bij,bkj->bki", Rc, kp.double()) + tc[:, None, :]
        if st.one_d:
            G = int(2 * ref.r / ref.s_z + 1)
            off = torch.zeros(G, 3, dtype=torch.float64)
            off[:, 2] = (torch.arange(G, dtype=torch.float64) - (G - 1) / 2.0) * ref.s_z
        else:
            G = int(2 * ref.r / ref.s + 1)
            off = OP.centred_grid(G, ref.s)
        cand = (moved[:, :, None, :] + off[None, None]).float()
        C = cand.shape[2]
        trows = OP.group_rows(cand.reshape(B, ref.K * C, 3), xt, f_tgt, ref.d, ref.ns)
        tgt_dfe = st.DFE(trows.reshape(B, ref.K, C, ref.ns, -1), src=False)
        if st.one_d:
            vcp = st.cpg(src_dfe, tgt_dfe, cand)
        else:
            vcp = st.cpg(src_dfe.unsqueeze(2), tgt_dfe.contiguous().view(B, ref.K, 32, C), cand, ref.r, ref.s)
        Rs, ts = [], []
        for b in range(B):
            Rb, tb, _ = OP.paper_pose(kp[b].double().T.numpy(), vcp[b].detach().double().T.numpy(),
                                      w[b].detach().double().numpy(), ref.inlier_ratio)
            Rs.append(torch.from_numpy(Rb))
            ts.append(torch.from_numpy(tb))
        Rc, tc = torch.stack(Rs), torch.stack(ts)
        out.append(dict(keypts=kp, vcp=vcp, weights=w, R=Rc, t=tc, topk=top, cand=cand, score=score))
    return out


def _condition(ref, features, fe_scale=300.0, wl_scale=10.0, target_std=2.0, cpg_scale=30.0):
    """The default init made well-conditioned for a gradient comparison, as dvcp.synthetic's
    condition_weights does for the reference network (every op and shape stays the checker's).
    Untouched, the extractor's features are 0.12 +- 1.4e-5 over the cloud (two hundred fp32 steps),
    the key points' weights agree to 3e-8 and both CPGs' softmaxes are flat: every vcp is its key
    point moved rigidly, the pose fit is exact to 1e-6, the rejection cut is decided by rounding and
    the weighting layers' true gradients are 1e-15 -- nothing to compare.  Making the weighting
    layer alone steeper only amplifies the extractor's own rounding (measured: weights 3e-3 apart
    between the GPU and the checker, weighting gradients 2e-2).  So the frozen extractor's first
    convolution is scaled by ``fe_scale`` (features +- 4.5e-3); each weighting layer's fc1 / fc2
    weights are scaled by ``wl_scale`` and fc3 is set so that the logit has mean 0 and std
    ``target_std`` on ``features()`` (P x 32, evaluated after the extractor is scaled); each CPG's
    conv1 and conv3 weights are scaled by ``cpg_scale``."""
    with torch.no_grad():
        ref.FE.sa1.mlp_convs[0].weight *= fe_scale
        feats = features()
        for st in ref.stages:
            st.cpg.conv1.weight *= cpg_scale
            st.cpg.conv3.weight *= cpg_scale
            wl = st.WL
            wl.fc1.weight *= wl_scale
            wl.fc2.weight *= wl_scale
            h = torch.relu(wl.bn2(wl.fc2(torch.relu(wl.bn1(wl.fc1(feats))))))
            z = h @ wl.fc3.weight.t()
            scale = target_std / float(z.std())
            wl.fc3.weight *= scale
            wl.fc3.bias.fill_(-float(z.mean()) * scale)


def _pair(cuda, seed, train_heads=True):
    from oracle import paper as OP
    import oracle as O
    import dvcp
    from dvcp.synthetic import make_pairs
    B, N = 1, 512
    src, tgt, R_gt, t_gt = make_pairs(B, N, seed=seed)
    torch.manual_seed(8)
    ref = OP.DeepVCPPaper(use_normal=False, **CFG).eval()
    _randomize_bn(ref)
    ref.FE.requires_grad_(False)
    mine = dvcp.paper.DeepVCPPaper(use_normal=False, train_heads=train_heads, **CFG).eval()
    starts = torch.stack([mine.FE.draw_starts(B, N), mine.FE.draw_starts(B, N)])

    def features():
        with O.fps_starts(list(starts[0])):
            return ref.FE(src).reshape(-1, 32)

    _condition(ref, features)
    mine.load_state_dict(ref.state_dict())
    mine.to(cuda)
    mine.FE.requires_grad_(False)
    return ref, mine, src, tgt, R_gt, t_gt, starts


def test_paper_head_train_step_vs_oracle(cuda):
    """DeepVCPPaper(train_heads=True): forward, the paper loss summed over both stages, backward, one
    Adam step, against the checker's own step (test_paper_model_with_duplication_vs_oracle's recipe
    at B = 1, N = 512, K = 8; the GPU run from the checker's key points, the extractor frozen on both
    sides)."""
    from oracle import paper as OP
    import oracle as O
    import dvcp
    ref, mine, src, tgt, R_gt, t_gt, starts = _pair(cuda, seed=66)
    B, K = 1, CFG["K"]
    order = list(starts[0]) + list(starts[1])
    with torch.no_grad(), O.fps_starts(order):
        plain = ref(src, tgt, R_gt, torch.zeros(1, 3))
    with O.fps_starts(order):
        want = _checker_forward(ref, src, tgt, R_gt, torch.zeros(1, 3))
    loss_o = 0.0
    for si, (st, pl) in enumerate(zip(want, plain)):
        assert torch.equal(st["vcp"].detach(), pl["vcp"]) and torch.equal(st["weights"].detach(), pl["weights"]), si
        assert torch.equal(st["topk"], pl["topk"]) and torch.equal(st["R"], pl["R"]), si
        assert st["vcp"].requires_grad and st["weights"].requires_grad
        # the rejection cut (6 of 8 kept) is no near tie under the first solve
        x = st["keypts"][0].double().T.numpy()
        y = st["vcp"][0].detach().double().T.numpy()
        R1, t1 = OP.weighted_rigid_transform(x, y, st["weights"][0].detach().double().numpy())
        res = np.sort(np.linalg.norm(R1 @ x + t1[:, None] - y, axis=0))
        m = int(0.8 * K)
        gap = (res[m] - res[m - 1]) / res[m]
        print(f"stage {si}: rejection gap {gap:.2e} of the first dropped residual {res[m]:.2e}")
        assert gap > 1e-6 and res[m] > 1e-3, (si, gap, res[m])   # and the residuals are no rounding noise
        l, _, _ = OP.deepvcp_loss_paper_torch(st["keypts"].double().permute(0, 2, 1), st["vcp"].double().permute(0, 2, 1),
                                              st["weights"].double(), R_gt, t_gt.reshape(B, 3), 0.5, inlier_ratio=0.8)
        loss_o = loss_o + l
    loss_o.backward()

    def run():
        got = mine(src.to(cuda), tgt.to(cuda), R_gt.to(cuda), torch.zeros(1, 3), starts=starts,
                   keypoint_idx=[st["topk"] for st in want])
        loss = 0.0
        for st in got:
            loss = loss + dvcp.paper.deepVCP_loss_paper(st["keypts"], st["vcp"], st["weights"], R_gt.to(cuda),
                                                        t_gt.to(cuda), 0.5, inlier_ratio=0.8)[0]
        return got, loss

    got, loss = run()
    for st in got:
        assert st["vcp"].requires_grad and st["weights"].requires_grad and not st["keypts"].requires_grad
        # the K rows' scores recomputed differentiably are the gathered full scores, bit for bit
        assert torch.equal(st["weights"].detach(), torch.gather(st["score"], 1, st["topk"]))
    loss.backward()
    print(f"loss {float(loss.detach()):.6f} (checker {float(loss_o.detach()):.6f})")
    errs, scale = {}, {}
    mine_p = dict(mine.stages.named_parameters())
    for name, p in ref.stages.named_parameters():
        assert name.split(".")[1] in ("WL", "DFE", "cpg") and p.grad is not None, name
        zero = name.endswith("cpg.conv3.bias") or (".DFE." in name and name.endswith(".bias"))
        errs[name] = _rel(mine_p[name].grad, p.grad, 1e-3 if zero else 1e-30)
        scale[name] = float(p.grad.abs().max())
        assert torch.isfinite(mine_p[name].grad).all(), name
        if zero:   # floored because the true gradient is zero: the checker's own value says so
            assert scale[name] < 1e-6, (name, scale[name])
    print("checker gradient scales:", {k: f"{v:.1e}" for k, v in scale.items()})
    print("GPU gradient scales:", {k: f"{float(mine_p[k].grad.abs().max()):.1e}" for k in scale})
    torch.testing.assert_close(loss.detach().cpu(), loss_o.detach(), rtol=1e-4, atol=0)
    _check("paper head training step", errs, 1e-3)
    assert min(scale["0.cpg.conv1.weight"], scale["1.cpg.conv1.weight"], scale["0.WL.fc1.weight"],
               scale["1.WL.fc1.weight"]) > 1e-5    # the comparison is not vacuous
    assert all(p.grad is None for p in mine.FE.parameters())
    opt = torch.optim.Adam([p for p in mine.parameters() if p.requires_grad], lr=1e-3)
    before = mine.stages[1].cpg.conv1.weight.detach().clone()
    opt.step()
    assert not torch.equal(before, mine.stages[1].cpg.conv1.weight.detach())
    _, loss2 = run()
    assert torch.isfinite(loss2)


def test_train_heads_guards(cuda):
    ref, mine, src, tgt, R_gt, _, starts = _pair(cuda, seed=66)
    args = (src.to(cuda), tgt.to(cuda), R_gt.to(cuda), torch.zeros(1, 3))
    # a trainable extractor parameter is refused before any launch
    mine.FE.fc.bias.requires_grad_(True)
    with pytest.raises(NotImplementedError, match=r"extractor must be frozen \(model.FE.requires_grad_\(False\)\)"):
        mine(*args, starts=starts)
    mine.FE.requires_grad_(False)
    # train_heads=False under autograd: today's outputs, nothing carries a gradient
    mine.train_heads = False
    on = mine(*args, starts=starts)
    with torch.no_grad():
        off = mine(*args, starts=starts)
    for a, b in zip(on, off):
        for k in ("vcp", "weights", "R", "t", "keypts", "score", "src_dfe", "tgt_dfe"):
            assert torch.equal(a[k], b[k]) and not a[k].requires_grad, k
    # with the switch on, no_grad is the same inference
    mine.train_heads = True
    with torch.no_grad():
        off2 = mine(*args, starts=starts)
    assert all(torch.equal(a["vcp"], b["vcp"]) and not a["vcp"].requires_grad for a, b in zip(off2, off))
    # and the recorded forward computes the same values
    rec = mine(*args, starts=starts)
    for a, b in zip(rec, off):
        assert a["vcp"].requires_grad and torch.equal(a["vcp"].detach(), b["vcp"])
        assert torch.equal(a["weights"].detach(), b["weights"]) and torch.equal(a["R"], b["R"])
    with pytest.raises(NotImplementedError, match="training mode"):
        mine.train()(*args, starts=starts)
