"""Paper mode under batch-statistics BatchNorm (``bn_train=True`` and ``.train()``): the weighting
layer's own entry points (dvcp_weighting_bn_stats / _forward / _backward, csrc/paper_wl_train.hip)
against the checker's PaperWeighting in train mode (oracle/paper.py, fp64); the paper's first set
abstraction (3[+3] -> 32 -> 32) through ``batchnorm.train_forward`` / ``train_backward`` against the
checker's PointNetSetAbstraction in train mode; and DeepVCPPaper(train_heads=True, bn_train=True) after
``model.train(); model.FE.eval()`` (batch-statistics heads over a frozen-BN extractor) against the
checker's own step in the same state.

Bars.  Weighting layer: test_weighting_backward_vs_oracle's 1e-4 of each tensor's maximum (scores, d
feat, every parameter gradient); running mean / variance after the call rtol 1e-4 (atol 1e-6), as
test_sa_batch_stats_train_vs_oracle.  fc1.bias and fc2.bias feed a BN layer: the batch mean removes them,
their true gradient is zero and both sides hold summation noise, so they are compared at their weight
gradient's scale with 5e-2 (that test's conv.b rule).  Set abstraction: that test's bars (forward and
running statistics 1e-4, gradients 1e-3, conv.b as above).  Whole step: loss rtol 1e-4, parameter
gradients 1e-3 of each tensor's maximum, floored where the true gradient is zero (test_gpu_paper_train.py's
tensors, and the two linear biases under each BN layer at their weight gradient's scale)."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WL_NAMES = [(m, p) for m in ("fc1", "bn1", "fc2", "bn2", "fc3") for p in ("weight", "bias")]
WL_BUFFERS = [(m, b) for m in ("bn1", "bn2") for b in ("running_mean", "running_var")]


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


def _buffers_close(mine, ref, what):
    for (name, bm), (_, br) in zip(mine.named_buffers(), ref.named_buffers()):
        if name.endswith("num_batches_tracked"):
            assert int(bm) == int(br), (what, name, int(bm), int(br))
        else:
            print(f"{what}: {name} max |diff| {float((bm.cpu().double() - br.double()).abs().max()):.1e}")
            torch.testing.assert_close(bm.cpu().double(), br.double(), rtol=1e-4, atol=1e-6, msg=f"{what}: {name}")


# ----------------------------------------------------------------------------- weighting layer
@functools.lru_cache(maxsize=None)
def _wl_case(P, variant=""):
    """fp64 checker in train mode (randomised gamma, beta and running statistics), shared and
    read-only: the state before the call, the scores, every gradient, and the buffers after one call
    and after two.  Asserts that no ReLU pre-activation lies within 1e-6 of zero."""
    from oracle import paper as OP
    torch.manual_seed(11)
    ref = OP.PaperWeighting()
    _randomize_bn(ref, seed=12)
    ref = ref.double().train()
    with torch.no_grad():
        if variant == "gamma0":
            ref.bn1.weight[3] = 0.0
            ref.bn1.bias[3] = 0.05    # the unit stays on (a negative beta would mask it: d gamma = 0)
        if variant == "softplus":
            ref.fc3.bias += 25.0
    state = copy.deepcopy(ref.state_dict())
    g = torch.Generator().manual_seed(100 + P)
    feat = torch.randn(1, P, 32, generator=g)
    gs = torch.randn(1, P, generator=g)
    probe = copy.deepcopy(ref)
    with torch.no_grad():
        pre1 = probe.bn1(probe.fc1(feat.double().reshape(P, 32)))
        pre2 = probe.bn2(probe.fc2(torch.relu(pre1)))
        v = probe.fc3(torch.relu(pre2))
    margin = min(float(pre1.abs().min()), float(pre2.abs().min()))
    assert margin > 1e-6, f"P={P}: a ReLU pre-activation within {margin:.1e} of zero; choose another seed"
    if variant == "softplus":
        assert bool((v > 20).all())
    f_o = feat.double().clone().requires_grad_()
    score = ref(f_o)
    (score * gs.double()).sum().backward()
    gp = {n: getattr(getattr(ref, n[0]), n[1]).grad.clone() for n in WL_NAMES}
    after1 = copy.deepcopy(ref)
    with torch.no_grad():
        ref(feat.double())
    return dict(state=state, feat=feat, gs=gs, score=score.detach(), gfeat=f_o.grad, gp=gp, margin=margin,
                after1=after1, after2=ref)


def _wl_mine(c, cuda):
    import dvcp
    mine = dvcp.paper.PaperWeighting(bn_train=True)
    mine.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in c["state"].items()})
    return mine.to(cuda).train()


def _wl_errs(c, mine, cuda):
    mine.zero_grad()
    f_g = c["feat"].to(cuda).requires_grad_()
    score = mine(f_g)
    assert score.requires_grad
    (score * c["gs"].to(cuda)).sum().backward()
    assert all(torch.isfinite(t).all() for t in [score, f_g.grad] + [p.grad for p in mine.parameters()])
    errs = {"score": _rel(score, c["score"]), "d feat": _rel(f_g.grad, c["gfeat"])}
    for n in WL_NAMES:
        floor = 1e-30
        if n in (("fc1", "bias"), ("fc2", "bias")):   # true gradient zero: at the weight gradient's scale
            floor = float(c["gp"][(n[0], "weight")].abs().max())
        errs[".".join(n)] = _rel(getattr(getattr(mine, n[0]), n[1]).grad, c["gp"][n], floor)
    return errs, score.detach(), f_g.grad


WL_BOUND = {".".join(n): (5e-2 if n in (("fc1", "bias"), ("fc2", "bias")) else 1e-4) for n in WL_NAMES}
WL_BOUND.update({"score": 1e-4, "d feat": 1e-4})


@pytest.mark.parametrize("P", [2, 63, 64, 65, 1000, 16449])
def test_weighting_bn_train_vs_oracle(cuda, P):
    """PaperWeighting(bn_train=True).train() against the fp64 checker in train mode.  P = 2: biased and
    unbiased variance differ by a factor of 2; 63, 64, 65: around the 64-row tile; 1000: several
    tiles, the last one partial; 16449 = 257 tiles + 1 row: 256 workgroups, the first two walk two
    tiles and the fold sees 256 partial rows.  Then the running statistics after one call and after
    two, and the same bits from a second module in the same state."""
    c = _wl_case(P)
    mine = _wl_mine(c, cuda)
    errs, score, gfeat = _wl_errs(c, mine, cuda)
    print(f"smallest |ReLU pre-activation| {c['margin']:.1e}")
    _check(f"weighting bn train P={P}", errs, WL_BOUND)
    _buffers_close(mine, c["after1"], f"P={P} after one call")
    assert int(mine.bn1.num_batches_tracked) == int(mine.bn2.num_batches_tracked) == 1
    # a second module in the same starting state: the same bits everywhere
    twin = _wl_mine(c, cuda)
    _, score2, gfeat2 = _wl_errs(c, twin, cuda)
    assert torch.equal(score, score2) and torch.equal(gfeat, gfeat2)
    for a, b in zip(mine.parameters(), twin.parameters()):
        assert torch.equal(a.grad, b.grad)
    for a, b in zip(mine.buffers(), twin.buffers()):
        assert torch.equal(a, b)
    # under no_grad: the same scores, nothing recorded, the running statistics move again
    with torch.no_grad():
        plain = mine(c["feat"].to(cuda))
    assert not plain.requires_grad and torch.equal(plain, score)
    _buffers_close(mine, c["after2"], f"P={P} after two calls")
    assert int(mine.bn1.num_batches_tracked) == 2


@pytest.mark.parametrize("variant", ["gamma0", "softplus"])
def test_weighting_bn_train_variants(cuda, variant):
    """gamma0: bn1.weight[3] = 0 (the eval path's fold (W s) x cannot express xhat there; d gamma is
    still sum g xhat).  softplus: fc3.bias + 25, every row on the forward's v > 20 branch."""
    c = _wl_case(65, variant)
    mine = _wl_mine(c, cuda)
    errs, _, _ = _wl_errs(c, mine, cuda)
    _check(f"weighting bn train {variant}", errs, WL_BOUND)
    if variant == "gamma0":
        assert float(c["gp"][("bn1", "weight")][3].abs()) > 1e-6   # the comparison is not vacuous
    _buffers_close(mine, c["after1"], variant)


def test_weighting_bn_momentum_none_and_frozen(cuda):
    """momentum = None (cumulative average) and a frozen layer under features that need a gradient:
    batch statistics still, d feat within the bar, no parameter gradient."""
    from oracle import paper as OP
    c = _wl_case(65)
    ref = OP.PaperWeighting().double().train()
    ref.load_state_dict(c["state"])
    mine = _wl_mine(c, cuda)
    for m in (ref, mine):
        m.bn1.momentum = m.bn2.momentum = None
    with torch.no_grad():
        for _ in range(2):
            ref(c["feat"].double())
            mine(c["feat"].to(cuda))
    _buffers_close(mine, ref, "momentum None, two calls")
    frozen = _wl_mine(c, cuda).requires_grad_(False)
    x = c["feat"].to(cuda).requires_grad_()
    (frozen(x) * c["gs"].to(cuda)).sum().backward()
    assert all(p.grad is None for p in frozen.parameters()) and _rel(x.grad, c["gfeat"]) <= 1e-4
    assert int(frozen.bn1.num_batches_tracked) == 1


def test_weighting_bn_edges(cuda):
    """P = 1 raises as torch does, before any entry point; P = 0; the mode sums are d beta | d gamma;
    two calls and a null grad_feat give identical bits; eval mode is the eval path's bits."""
    import dvcp
    from dvcp import _lib, batchnorm, ops
    c = _wl_case(65)
    mine = _wl_mine(c, cuda)
    calls = []
    real = _lib.call

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)

    ops.call, keep = spy, ops.call
    try:
        with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
            mine(torch.zeros(1, 1, 32, device=cuda))
        assert calls == [] and int(mine.bn1.num_batches_tracked) == 0
    finally:
        ops.call = keep
    # P = 0 at every entry point
    rows0 = torch.zeros(0, 32, device=cuda)
    score0, st0 = batchnorm.weighting_train_forward(mine, rows0)
    assert score0.shape == (0,) and int(mine.bn1.num_batches_tracked) == 0
    pack, stat = st0["pack"], st0["bnstat"]
    assert pack.shape == (ops.WEIGHTING_BN_NPARAMS,) == (int(_lib.load().dvcp_weighting_bn_nparams()),)
    for layer, C in ((1, 16), (2, 8)):
        s = ops.weighting_bn_stats(rows0, pack, layer)
        assert s.shape == (2, C) and float(s.abs().max()) == 0.0
        s = ops.weighting_bn_backward(rows0, pack, stat, torch.zeros(0, device=cuda), layer)
        assert s.shape == (2, C) and float(s.abs().max()) == 0.0
    gp, gf = ops.weighting_bn_backward(rows0, pack, stat, torch.zeros(0, device=cuda), 0)
    assert gf.shape == (0, 32) and gp.shape == (673,) and float(gp.abs().max()) == 0.0
    assert ops.weighting_bn_forward(rows0, pack).shape == (0,)
    grads, gf = batchnorm.weighting_train_backward(mine, st0, torch.zeros(0, device=cuda), True)
    assert all(float(g.abs().max()) == 0.0 for g in grads) and gf.shape == (0, 32)
    # the raw passes on 65 rows: statistics against fp64 torch, then identical bits
    rows = c["feat"].to(cuda).reshape(65, 32).contiguous()
    gs = c["gs"].to(cuda).reshape(65)
    score, st = batchnorm.weighting_train_forward(mine, rows)
    z1 = c["feat"].double().reshape(65, 32) @ c["state"]["fc1.weight"].t() + c["state"]["fc1.bias"]
    mean, rstd = st["bnstat"][:16].cpu().double(), st["bnstat"][16:32].cpu().double()
    torch.testing.assert_close(mean, z1.mean(0), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(rstd, torch.rsqrt(z1.var(0, unbiased=False) + 1e-5), rtol=1e-5, atol=0)
    one = batchnorm.weighting_train_backward(mine, st, gs, True)
    two = batchnorm.weighting_train_backward(mine, st, gs, True)
    nof = batchnorm.weighting_train_backward(mine, st, gs, False)
    assert torch.equal(one[1], two[1]) and nof[1] is None
    for a, b, d in zip(one[0], two[0], nof[0]):
        assert torch.equal(a, b) and torch.equal(a, d)
    names = dict(zip(WL_NAMES, one[0]))
    for n in (("bn1", "weight"), ("bn1", "bias"), ("bn2", "weight"), ("bn2", "bias")):   # B_l and A_l
        assert _rel(names[n], c["gp"][n]) <= 1e-4, n
    # eval mode with the flag: the eval path's bits (the folded kernel), nothing updated
    plain = dvcp.paper.PaperWeighting().to(cuda).eval()
    plain.load_state_dict(mine.state_dict())
    before = copy.deepcopy(mine.state_dict())
    with torch.no_grad():
        assert torch.equal(mine.eval()(c["feat"].to(cuda)), plain(c["feat"].to(cuda)))
    assert all(torch.equal(v, before[k]) for k, v in mine.state_dict().items())
    assert list(plain.state_dict()) == list(mine.state_dict())
    with pytest.raises(NotImplementedError, match="training mode"):
        plain.train()(c["feat"].to(cuda))


@pytest.mark.parametrize("P", [1, 65])   # one row; a full 64-row tile and a one-row tile
def test_weighting_backward_eval_and_identity_bn_same_bits(cuda, P):
    """The eval and the batch-statistics instance of the one backward kernel on the same numbers: the
    eval pack of unfolded fc1-fc3, and the train pack with scale = 1, shift = 0 under mean = 0, rstd = 1,
    A/M = B/M = 0.  The BN path then computes z * 1 + 0 and 1 * ((g - 0) - xhat * 0), which reproduce z
    and g exactly up to the sign of a zero, so every gradient is equal (torch.equal ignores that sign)."""
    from dvcp import ops
    gen = torch.Generator().manual_seed(700 + P)
    w1, b1 = torch.randn(16, 32, generator=gen) * 0.3, torch.randn(16, generator=gen)
    w2, b2 = torch.randn(8, 16, generator=gen) * 0.3, torch.randn(8, generator=gen)
    w3, b3 = torch.randn(8, generator=gen) * 0.3, torch.randn(1, generator=gen)
    feat = torch.randn(P, 32, generator=gen).to(cuda)
    g = torch.randn(P, generator=gen).to(cuda)
    eval_pack = torch.cat([w1.reshape(-1), b1, w2.reshape(-1), b2, w3, b3]).to(cuda)
    train_pack = torch.cat([w1.reshape(-1), b1, torch.ones(16), torch.zeros(16), w2.reshape(-1), b2, torch.ones(8),
                            torch.zeros(8), w3, b3]).to(cuda)
    assert eval_pack.numel() == ops.WEIGHTING_NPARAMS and train_pack.numel() == ops.WEIGHTING_BN_NPARAMS
    bnstat = torch.zeros(ops.WEIGHTING_BN_NSTAT, dtype=torch.float64, device=cuda)
    bnstat[16:32] = 1.0            # bn1: mean | rstd | A/M | B/M, 16 each
    bnstat[64 + 8:64 + 16] = 1.0   # bn2: the same, 8 each
    gp_e, gf_e = ops.weighting_backward(feat, eval_pack, g)
    gp_b, gf_b = ops.weighting_bn_backward(feat, train_pack, bnstat, g, 0)
    assert float(gp_e.abs().max()) > 0.0   # d b3 = sum g softplus'(v) at the least
    assert torch.equal(gp_e, gp_b)
    assert torch.equal(gf_e, gf_b)


# ------------------------------------------------------------- the paper's sa1, batch statistics
def _near_tie_mask(ref, xyz, feat, S, radius, ns, start, rel=1e-5):
    """test_gpu_train.py's helper: (B, C, S) True where a channel's maximum over the grouped rows is
    within ``rel`` of the best row of a different point (fp64 values of ``ref``, a deep copy in
    double): there the two fp32 pipelines may pick different arg-max rows."""
    import oracle as O
    with torch.no_grad(), O.fps_starts([start]):
        _, grouped, gidx = O.sample_and_group(S, radius, ns, xyz.permute(0, 2, 1),
                                              None if feat is None else feat.permute(0, 2, 1), returnidx=True)
        x = grouped.permute(0, 3, 2, 1)
        for conv, bn in zip(ref.mlp_convs, ref.mlp_bns):
            x = torch.relu(bn(conv(x.double())))
        mx, am = x.max(2)                                         # (B, C, S)
        pid = gidx.permute(0, 2, 1)                               # (B, ns, S): point of each row
        pid_am = torch.gather(pid.unsqueeze(1).expand(-1, x.shape[1], -1, -1), 2, am.unsqueeze(2))
        other = torch.where(pid.unsqueeze(1) != pid_am, x, torch.full_like(x, -1.0)).max(2).values
        return (mx > 0) & (mx - other <= rel * mx)


@pytest.mark.parametrize("D", [0, 3])
def test_paper_sa1_batch_stats_train_vs_oracle(cuda, D):
    """The paper's first set abstraction (3 + D -> 32 -> 32) in training mode through
    batchnorm.train_forward / train_backward (the lane-per-entry passes of csrc/sa_bn.hip; the
    matrix-core path does not take this table): test_sa_backward_paper_sa1_vs_oracle's shape and
    near-tie handling, test_sa_batch_stats_train_vs_oracle's bars."""
    import oracle as O
    import dvcp
    from dvcp import batchnorm, ops
    g = torch.Generator().manual_seed(410 + D)
    B, N, S, ns, radius = 2, 1024, 128, 32, 0.12
    xyz = torch.rand(B, 3, N, generator=g) * 0.6 - 0.3
    feat = None
    if D:
        feat = torch.randn(B, 3, N, generator=g)
        feat = feat / feat.norm(dim=1, keepdim=True)
    torch.manual_seed(11)
    ref = O.PointNetSetAbstraction(S, radius, ns, 3 + D, [32, 32])
    _randomize_bn(ref)
    ref.train()
    mine = dvcp.pointnet2_utils.PointNetSetAbstraction(S, radius, ns, 3 + D, [32, 32])
    mine.load_state_dict(ref.state_dict())
    mine.to(cuda).train()
    start = torch.randint(0, N, (B,), generator=g)
    G = torch.randn(B, 32, S, generator=g)
    near = _near_tie_mask(copy.deepcopy(ref).double().train(), xyz.double(), None if feat is None else feat.double(), S,
                          radius, ns, start)
    G[near] = 0.0
    with O.fps_starts([start]):
        _, out_o = ref(xyz, feat)                  # fp32, batch statistics
    (out_o * G).sum().backward()

    x, f = xyz.to(cuda), (None if feat is None else feat.to(cuda))
    _, ctr = ops.fps(x, S, start.to(cuda), pdim=2)
    count, lst, _ = ops.ball_query(x, ctr, radius, ns, pdim=2, cdim_pts=2)
    out, st = batchnorm.train_forward(mine, x, ctr, f, count, lst, ns, keep_zrows=True)
    assert not st.get("mfma")
    torch.testing.assert_close(out.permute(0, 2, 1).cpu(), out_o.detach(), rtol=1e-4, atol=1e-4)
    for bm, br in zip(mine.mlp_bns, ref.mlp_bns):
        torch.testing.assert_close(bm.running_mean.cpu(), br.running_mean, rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(bm.running_var.cpu(), br.running_var, rtol=1e-4, atol=1e-6)
        assert int(bm.num_batches_tracked) == int(br.num_batches_tracked) == 1
    lay = dict(pts=x, ctr=ctr, feat=f, count=count, lst=lst, ns=ns, bn=st)
    gp, gF = batchnorm.train_backward(mine, lay, G.permute(0, 2, 1).float().to(cuda), want_feat_grad=False)
    assert gF is None
    o, errs, bound = 0, {}, {}
    for i, (conv, bn) in enumerate(zip(ref.mlp_convs, ref.mlp_bns)):
        co, ci = conv.weight.shape[:2]
        wscale = float(conv.weight.grad.abs().max())
        for name, want, n, floor, tol in (("conv.w", conv.weight.grad.reshape(co, ci), co * ci, 1e-30, 1e-3),
                                          ("conv.b", conv.bias.grad, co, wscale, 5e-2),
                                          ("bn.w", bn.weight.grad, co, 1e-30, 1e-3),
                                          ("bn.b", bn.bias.grad, co, 1e-30, 1e-3)):
            errs[f"{i}.{name}"] = _rel(gp[o:o + n].view(want.shape), want, floor)
            bound[f"{i}.{name}"] = tol
            o += n
    print(f"D={D}: near-tie pairs left out: {int(near.sum())} of {near.numel()}")
    _check(f"paper sa1 batch statistics D={D}", errs, bound)


# ------------------------------------------------------------------------- the whole network
CFG = dict(K=8, r=0.4, s=0.4, s_z=0.25, d=1.0, npoints=(128, 32, 8))   # a 3^3 grid and a 4-point z line


def _checker_forward(ref, src, tgt, R_init, t_init):
    """oracle/paper.py DeepVCPPaper.forward, statement for statement, for a forward that records
    autograd (tests/test_gpu_paper_train.py's helper): the checker's numpy pose solve takes ``vcp`` and
    ``w`` detached; nothing else differs."""
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
        out.append(dict(keypts=kp, vcp=vcp, weights=w, R=Rc, t=tc, topk=top, cand=cand, score=score, feat=f_src))
    return out


def _wl_pre(wl, feats):
    """The weighting layer's two ReLU pre-activations and its logit under batch statistics (fp64, no
    buffer touched)."""
    Fn = torch.nn.functional
    wl = copy.deepcopy(wl).double()
    x = feats.double()
    with torch.no_grad():
        pre1 = Fn.batch_norm(wl.fc1(x), None, None, wl.bn1.weight, wl.bn1.bias, True, 0.0, wl.bn1.eps)
        pre2 = Fn.batch_norm(wl.fc2(torch.relu(pre1)), None, None, wl.bn2.weight, wl.bn2.bias, True, 0.0, wl.bn2.eps)
        return pre1, pre2, torch.relu(pre2) @ wl.fc3.weight.t()


def _condition(ref, features, fe_scale=3000.0, wl_scale=10.0, target_std=2.0, cpg_scale=30.0):
    """tests/test_gpu_paper_train.py::_condition with the weighting layers evaluated under batch
    statistics (the mode they run in here): the extractor's first convolution, fc1 / fc2 and each CPG's
    conv1 / conv3 scaled, fc3 set so that the logit has mean 0 and std ``target_std`` on ``features()``.
    ``fe_scale`` is 3000 here, not that test's 300.  Under batch statistics sum dz1 = 0, so d fc1.weight =
    sum dz1 (f - mean f)^T: with 300 a feature channel is its mean +- 4.8e-3 (means up to 0.14), the sum
    cancels 30-fold and the fp32 checker itself is 1.6e-3 of the tensor's maximum away from its own fp64
    run (stage 1: a ReLU unit 1.5e-5 from its kink flips between the two precisions).  With 3000 the
    channels spread +- 5.7e-2 and the fp32 checker is within 5e-6 of fp64 (``_step_case`` asserts 1e-4)."""
    with torch.no_grad():
        ref.FE.sa1.mlp_convs[0].weight *= fe_scale
        feats = features()
        for st in ref.stages:
            st.cpg.conv1.weight *= cpg_scale
            st.cpg.conv3.weight *= cpg_scale
            wl = st.WL
            wl.fc1.weight *= wl_scale
            wl.fc2.weight *= wl_scale
            z = _wl_pre(wl, feats)[2].float()
            scale = target_std / float(z.std())
            wl.fc3.weight *= scale
            wl.fc3.bias.fill_(-float(z.mean()) * scale)


@functools.lru_cache(maxsize=None)
def _step_case(seed=66):
    """The checker's step at B = 2, N = 512, K = 8 after ``ref.train(); ref.FE.eval()`` with the
    extractor frozen: the state before the step, the outputs, the loss, every head gradient and the
    buffers after the step.  Asserts the conditions the comparison rests on."""
    from oracle import paper as OP
    import oracle as O
    from dvcp.synthetic import make_pairs
    B, N, K = 2, 512, CFG["K"]
    src, tgt, R_gt, t_gt = make_pairs(B, N, seed=seed)
    torch.manual_seed(8)
    ref = OP.DeepVCPPaper(use_normal=False, **CFG).eval()
    _randomize_bn(ref)
    ref.FE.requires_grad_(False)
    g = torch.Generator().manual_seed(seed)
    starts = torch.stack([torch.stack([torch.randint(0, n, (B,), generator=g) for n in (N, 128, 32)])
                          for _ in range(2)])
    order = list(starts[0]) + list(starts[1])

    def features():
        with O.fps_starts(list(starts[0])):
            return ref.FE(src).reshape(-1, 32)

    _condition(ref, features)
    ref.train()
    ref.FE.eval()
    state = copy.deepcopy(ref.state_dict())
    with O.fps_starts(order):
        want = _checker_forward(ref, src, tgt, R_gt, torch.zeros(1, 3))
    loss_o = 0.0
    for si, (st, stage) in enumerate(zip(want, ref.stages)):
        assert st["vcp"].requires_grad and st["weights"].requires_grad
        wl0 = OP.PaperWeighting()
        wl0.load_state_dict({k[len(f"stages.{si}.WL."):]: v for k, v in state.items() if k.startswith(f"stages.{si}.WL.")})
        pre1, pre2, _ = _wl_pre(wl0, st["feat"].detach().reshape(-1, 32))
        margin = min(float(pre1.abs().min()), float(pre2.abs().min()))
        print(f"stage {si}: smallest |weighting ReLU pre-activation| {margin:.1e}")
        assert margin > 1e-5, (si, margin)   # fp32 carries rstd ~ 1e2 here: a wider berth than the 1e-6 elsewhere
        # the comparison is well posed: on these features the fp32 checker's weighting gradients (a probe
        # gradient on the K key points' scores) are its own fp64 run's within 1e-4
        probe = torch.zeros(B, N).scatter_(1, st["topk"], torch.randn(B, K, generator=g))
        runs = []
        for dt in (torch.float32, torch.float64):
            m = copy.deepcopy(wl0).to(dt).train()
            (m(st["feat"].detach().to(dt)) * probe.to(dt)).sum().backward()
            runs.append({n: p.grad for n, p in m.named_parameters() if n not in ("fc1.bias", "fc2.bias")})
        own = max(_rel(runs[0][n], runs[1][n]) for n in runs[0])
        print(f"stage {si}: fp32 checker against fp64 on the weighting layer's gradients {own:.1e}")
        assert own < 1e-4, (si, own)
        for b in range(B):   # the rejection cut (6 of 8 kept) is no near tie under the first solve
            x = st["keypts"][b].double().T.numpy()
            y = st["vcp"][b].detach().double().T.numpy()
            R1, t1 = OP.weighted_rigid_transform(x, y, st["weights"][b].detach().double().numpy())
            res = np.sort(np.linalg.norm(R1 @ x + t1[:, None] - y, axis=0))
            m = int(0.8 * K)
            gap = (res[m] - res[m - 1]) / res[m]
            print(f"stage {si} pair {b}: rejection gap {gap:.2e} of the first dropped residual {res[m]:.2e}")
            assert gap > 1e-6 and res[m] > 1e-3, (si, b, gap, res[m])
        l, _, _ = OP.deepvcp_loss_paper_torch(st["keypts"].double().permute(0, 2, 1), st["vcp"].double().permute(0, 2, 1),
                                              st["weights"].double(), R_gt, t_gt.reshape(B, 3), 0.5, inlier_ratio=0.8)
        loss_o = loss_o + l
    loss_o.backward()
    return dict(ref=ref, state=state, src=src, tgt=tgt, R_gt=R_gt, t_gt=t_gt, starts=starts, want=want,
                loss=loss_o.detach())


def _step_mine(c, cuda, **flags):
    import dvcp
    mine = dvcp.paper.DeepVCPPaper(use_normal=False, bn_train=True, **flags, **CFG)
    mine.load_state_dict(c["state"])
    mine.to(cuda)
    mine.FE.requires_grad_(False)
    mine.train()
    mine.FE.eval()
    return mine


def _step_run(c, mine, cuda):
    import dvcp
    got = mine(c["src"].to(cuda), c["tgt"].to(cuda), c["R_gt"].to(cuda), torch.zeros(1, 3), starts=c["starts"],
               keypoint_idx=[st["topk"] for st in c["want"]])
    loss = 0.0
    for st in got:
        loss = loss + dvcp.paper.deepVCP_loss_paper(st["keypts"], st["vcp"], st["weights"], c["R_gt"].to(cuda),
                                                    c["t_gt"].to(cuda), 0.5, inlier_ratio=0.8)[0]
    return got, loss


def test_paper_bn_heads_train_step_vs_oracle(cuda):
    """``model.train(); model.FE.eval()`` on DeepVCPPaper(train_heads=True, bn_train=True): frozen-BN
    extractor, batch-statistics weighting layers over the B N = 1024 source rows of B = 2 pairs (the
    statistics span pairs), against the checker in the same state: loss, every head gradient (d loss
    / d weights reaches all rows through the BN backward), the buffers after the step (each WL's
    updated once, the extractor's untouched), then one Adam step and a second forward."""
    c = _step_case()
    ref = c["ref"]
    mine = _step_mine(c, cuda, train_heads=True)
    got, loss = _step_run(c, mine, cuda)
    for st, w in zip(got, c["want"]):
        assert st["vcp"].requires_grad and st["weights"].requires_grad and not st["keypts"].requires_grad
        assert not st["score"].requires_grad
        assert torch.equal(st["weights"].detach(), torch.gather(st["score"], 1, st["topk"]))
        print(f"scores: max |diff| {float((st['score'].cpu() - w['score'].detach()).abs().max()):.1e}")
        torch.testing.assert_close(st["score"].cpu(), w["score"].detach(), rtol=1e-4, atol=1e-4)
    loss.backward()
    print(f"loss {float(loss.detach()):.6f} (checker {float(c['loss']):.6f})")
    errs, scale = {}, {}
    mine_p = dict(mine.stages.named_parameters())
    ref_p = dict(ref.stages.named_parameters())
    for name, p in ref_p.items():
        assert p.grad is not None, name
        zero = name.endswith("cpg.conv3.bias") or (".DFE." in name and name.endswith(".bias"))
        floor = 1e-3 if zero else 1e-30
        if name.endswith(("WL.fc1.bias", "WL.fc2.bias")):   # under a BN layer: at the weight gradient's scale
            floor = float(ref_p[name[:-4] + "weight"].grad.abs().max())
        errs[name] = _rel(mine_p[name].grad, p.grad, floor)
        scale[name] = float(p.grad.abs().max())
        assert torch.isfinite(mine_p[name].grad).all(), name
        if zero:
            assert scale[name] < 1e-6, (name, scale[name])
    print("checker gradient scales:", {k: f"{v:.1e}" for k, v in scale.items()})
    torch.testing.assert_close(loss.detach().cpu(), c["loss"], rtol=1e-4, atol=0)
    bound = {k: (5e-2 if k.endswith(("WL.fc1.bias", "WL.fc2.bias")) else 1e-3) for k in errs}
    _check("paper bn-heads training step", errs, bound)
    assert min(scale["0.cpg.conv1.weight"], scale["1.cpg.conv1.weight"], scale["0.WL.fc1.weight"],
               scale["1.WL.fc1.weight"]) > 1e-5    # the comparison is not vacuous
    assert all(p.grad is None for p in mine.FE.parameters())
    _buffers_close(mine, ref, "after the step")
    for st in mine.stages:
        assert int(st.WL.bn1.num_batches_tracked) == int(st.WL.bn2.num_batches_tracked) == 1
    assert all(int(b) == 0 for n, b in mine.FE.named_buffers() if n.endswith("num_batches_tracked"))
    opt = torch.optim.Adam([p for p in mine.parameters() if p.requires_grad], lr=1e-3)
    before = mine.stages[1].WL.fc1.weight.detach().clone()
    opt.step()
    assert not torch.equal(before, mine.stages[1].WL.fc1.weight.detach())
    _, loss2 = _step_run(c, mine, cuda)
    assert torch.isfinite(loss2)
    assert int(mine.stages[0].WL.bn1.num_batches_tracked) == 2


def test_paper_bn_modes(cuda):
    """.eval() after training-mode forwards is the inference path's bits for the same state_dict; under
    no_grad in train mode the weights are the recorded forward's bits and the statistics move; the
    flag off refuses .train() with today's message on every class."""
    import dvcp
    c = _step_case()
    args = (c["src"].to(cuda), c["tgt"].to(cuda), c["R_gt"].to(cuda), torch.zeros(1, 3))
    mine = _step_mine(c, cuda, train_heads=True)
    rec, _ = _step_run(c, mine, cuda)
    with torch.no_grad():
        off = mine(*args, starts=c["starts"], keypoint_idx=[st["topk"] for st in c["want"]])
    for a, b in zip(rec, off):
        assert not b["weights"].requires_grad and torch.equal(a["weights"].detach(), b["weights"])
        assert torch.equal(a["vcp"].detach(), b["vcp"])
    assert int(mine.stages[0].WL.bn1.num_batches_tracked) == 2
    # train_heads off: inference in train mode, batch statistics still, nothing recorded
    mine.train_heads = False
    on = mine(*args, starts=c["starts"], keypoint_idx=[st["topk"] for st in c["want"]])
    assert all(not a["weights"].requires_grad and torch.equal(a["weights"], b["weights"]) for a, b in zip(on, off))
    assert int(mine.stages[1].WL.bn2.num_batches_tracked) == 3
    # .eval(): the inference path's bits for the same state_dict
    plain = dvcp.paper.DeepVCPPaper(use_normal=False, **CFG).to(cuda).eval()
    plain.load_state_dict(mine.state_dict())
    before = copy.deepcopy(mine.state_dict())
    with torch.no_grad():
        a, b = mine.eval()(*args, starts=c["starts"]), plain(*args, starts=c["starts"])
    for x, y in zip(a, b):
        for k in ("vcp", "weights", "R", "t", "keypts", "score", "topk"):
            assert torch.equal(x[k], y[k]), k
    assert all(torch.equal(v, before[k]) for k, v in mine.state_dict().items())
    # mixed: one stage's WL in eval mode keeps the K-row recomputation
    mine.train_heads = True
    mine.train()
    mine.FE.eval()
    mine.stages[0].WL.eval()
    got, _ = _step_run(c, mine, cuda)
    assert got[0]["weights"].requires_grad and got[1]["weights"].requires_grad
    assert int(mine.stages[0].WL.bn1.num_batches_tracked) == 3 and int(mine.stages[1].WL.bn1.num_batches_tracked) == 4
    # refusals: built without the flag, all four classes with BatchNorm refuse .train() with today's message
    with pytest.raises(NotImplementedError, match="DeepVCPPaper.forward in training mode"):
        plain.train()(*args, starts=c["starts"])
    x = torch.zeros(1, 3, 8, device=cuda)
    for mod, a in ((dvcp.paper.PointNetFeaturePropagation(35, [32, 32]), (x, x, x, torch.zeros(1, 32, 8, device=cuda))),
                   (dvcp.paper.PaperFeatExtraction(npoints=(16, 8, 4)), (args[0],)),
                   (dvcp.paper.PaperWeighting(), (torch.zeros(1, 4, 32, device=cuda),))):
        with pytest.raises(NotImplementedError, match=f"{type(mod).__name__}.forward in training mode"):
            mod.to(cuda).train()(*a)
