"""Paper mode under batch-statistics BatchNorm, the extractor's half (``bn_train=True`` and ``.train()``):
PointNetFeaturePropagation (dvcp_feature_propagation_bn_stats / _bn_backward, the template modes of
fp_bwd_kernel in csrc/paper_fe_bwd.hip), PaperFeatExtraction, and the whole DeepVCPPaper step with
every module in training mode, against the checker's modules (oracle/paper.py, torch modules in fp32)
in train mode.  The weighting layer and the paper's sa1 table are in test_gpu_paper_bn_train.py.

Bars (test_sa_batch_stats_train_vs_oracle's): forward within 1e-4; running mean / variance
after the call rtol 1e-4 (atol 1e-6); every W / gamma / beta gradient and input gradient within 1e-3 of
the tensor's max |grad|; conv and linear biases that feed a BN layer at their weight gradient's scale
with 5e-2 (their true gradient is zero; both sides hold summation noise); the mode sums A = sum g_a and
B = sum g_a xhat within 1e-4 of each vector's maximum.  Whole step: loss rtol 1e-4, parameter gradients
1e-3, or for a tensor that misses it max(1e-3, 4 x the fp32 checker's own spread on that tensor -- its
step run again with the batch rows in the other order), capped at 5e-3."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FP_TABLES = [(700, 32, 64, (32, 32)), (700, 0, 32, (32, 32, 32)), (3, 64, 64, (64, 64)), (1, 0, 32, (16,))]
FP_SEED = 4100   # chosen on the CPU: the checker alone meets the near-zero cap for every case below


def _rel(got, want, floor=1e-30):
    """max |got - want| / max(max |want|, floor)"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((got - want).abs().max()) / max(float(want.abs().max()), floor) if want.numel() else 0.0


def _check(what, errs, bound):
    """Every figure is printed before any is asserted."""
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


def _buffers_close(mine, ref, what, quiet=False):
    worst = 0.0
    for (name, bm), (_, br) in zip(mine.named_buffers(), ref.named_buffers()):
        if name.endswith("num_batches_tracked"):
            assert int(bm) == int(br), (what, name, int(bm), int(br))
        else:
            worst = max(worst, float((bm.cpu().double() - br.double()).abs().max()))
            torch.testing.assert_close(bm.cpu().double(), br.double(), rtol=1e-4, atol=1e-6, msg=f"{what}: {name}")
    print(f"{what}: running statistics max |diff| {worst:.1e}")


# ------------------------------------------------------------------------- feature propagation
@functools.lru_cache(maxsize=None)
def _fp_case(N2, D1, D2, mlp, N1, B=2, fc=False, coincident=False, salt=None):
    """One fp32 checker run in train mode (randomised gamma, beta, running statistics), shared and
    read-only: the state before the call, output rows, gradients, the buffers after, the rows with a
    ReLU pre-activation within 1e-5 of zero, and per BN layer A = sum g_a, B = sum g_a xhat from hooks
    on the BN outputs."""
    from oracle import paper as OP
    if N2 == 1 and D1 == 0 and B > 1 and salt is None:
        # one interpolation point and no points1: a cloud's rows are one row, so the statistics are those of
        # B distinct rows (M = 2 in effect) and g_a - A/M - xhat B/M cancels to eps / var of its size.  The
        # fp32 checker then carries its own error (measured up to 1.5e-3 of max |grad| against fp64 on d
        # points2): the inputs are drawn until the checker alone is within 1e-4 of its fp64 run.
        for salt in range(64):
            c = _fp_case(N2, D1, D2, mlp, N1, B, fc, coincident, salt)
            if c["own"] <= 1e-4:
                print(f"N2=1 B={B} N1={N1}: draw {salt}, fp32 checker against fp64 {c['own']:.1e}")
                return c
        raise AssertionError("no draw with a well-conditioned checker")
    g = torch.Generator().manual_seed(FP_SEED + 7 * N2 + D1 + 13 * N1 + 1000 * (salt or 0))
    torch.manual_seed(5)
    ref = OP.PointNetFeaturePropagation(D1 + D2, list(mlp))
    _randomize_bn(ref)
    ref.train()
    state = copy.deepcopy(ref.state_dict())
    lin = torch.nn.Linear(mlp[-1], 32) if fc else None
    xyz1 = torch.rand(B, 3, N1, generator=g) * 2 - 1
    if coincident:   # xyz2 = every fourth point of xyz1, as in the extractor (d = 0 up to rounding)
        xyz2 = xyz1[:, :, ::4].contiguous()
        assert xyz2.shape[2] == N2
    else:
        xyz2 = torch.rand(B, 3, N2, generator=g) * 2 - 1
    p1 = torch.randn(B, D1, N1, generator=g).requires_grad_() if D1 else None
    p2 = torch.randn(B, D2, N2, generator=g).requires_grad_()
    ys, gys = [], {}

    def hook(idx):
        def f(mod, i, o):
            ys.append(o.detach())
            o.register_hook(lambda gr: gys.__setitem__(idx, gr.detach()))
        return f

    handles = [bn.register_forward_hook(hook(i)) for i, bn in enumerate(ref.mlp_bns)]
    out = ref(xyz1, xyz2, p1, p2).permute(0, 2, 1)              # (B, N1, C) rows
    for h in handles:
        h.remove()
    if lin is not None:
        out = lin(out)
    near = torch.zeros(B, N1, dtype=torch.bool)
    for a in ys:                                                # (B, C, N1)
        near |= (a.abs() < 1e-5).any(1)
    G = torch.randn(out.shape, generator=g)
    (out * G).sum().backward()
    sums = []
    for i, bn in enumerate(ref.mlp_bns):                        # xhat = (y - beta) / gamma, in fp64
        gy = gys[i].double()
        xh = (ys[i].double() - bn.bias.detach().double()[None, :, None]) / bn.weight.detach().double()[None, :, None]
        sums.append(torch.stack([gy.sum((0, 2)), (gy * xh).sum((0, 2))]))
    grads = {}
    for i, (conv, bn) in enumerate(zip(ref.mlp_convs, ref.mlp_bns)):
        grads.update({f"{i}.conv.w": conv.weight.grad, f"{i}.conv.b": conv.bias.grad, f"{i}.bn.w": bn.weight.grad,
                      f"{i}.bn.b": bn.bias.grad})
    if lin is not None:
        grads.update({"fc.w": lin.weight.grad, "fc.b": lin.bias.grad})
    if p1 is not None:
        grads["p1"] = p1.grad
    grads["p2"] = p2.grad
    share = float(near.sum()) / max(B * N1, 1)
    assert share <= 0.01, f"{int(near.sum())} of {B * N1} rows near a ReLU kink: choose another seed"
    # one cloud, one interpolation point, no points1: every row is the same row, every z has variance 0 and
    # every weight gradient is zero analytically (sum dz = 0 times one x).  Such a tensor is compared at the
    # scale of a single un-cancelled term scale g x, with rstd = 1 / sqrt(eps).
    own = 0.0
    if N2 == 1 and D1 == 0 and B > 1:   # the same layer in fp64 (the interpolation of one point is that point)
        Fn = torch.nn.functional
        W = state["mlp_convs.0.weight"].double().requires_grad_()
        q2 = p2.detach().double().requires_grad_()
        bn0 = ref.mlp_bns[0]
        y = Fn.batch_norm(Fn.conv1d(q2.expand(B, D2, N1), W, state["mlp_convs.0.bias"].double()), None, None,
                          state["mlp_bns.0.weight"].double(), state["mlp_bns.0.bias"].double(), True, 0.0, bn0.eps)
        (torch.relu(y).permute(0, 2, 1) * G.double()).sum().backward()
        own = max(_rel(p2.grad, q2.grad), _rel(ref.mlp_convs[0].weight.grad, W.grad))
    term = None
    if B == 1 and N2 == 1 and D1 == 0:
        bn0 = ref.mlp_bns[0]
        term = float(G.abs().max()) * float(bn0.weight.detach().abs().max()) / bn0.eps ** 0.5 * float(p2.detach().abs().max())
    return dict(ref=ref, state=state, lin=lin, xyz1=xyz1, xyz2=xyz2, p1=p1, p2=p2, out=out.detach(), G=G, grads=grads,
                near=near, sums=sums, mlp=list(mlp), cin=D1 + D2, term=term, own=own)


def _fp_mine(c, cuda):
    import dvcp
    mine = dvcp.paper.PointNetFeaturePropagation(c["cin"], c["mlp"], bn_train=True)
    mine.load_state_dict(c["state"])
    lin = None if c["lin"] is None else copy.deepcopy(c["lin"]).to(cuda)
    if lin is not None:
        lin.zero_grad()
    return mine.to(cuda).train(), lin


def _fp_run(c, mine, lin, cuda):
    from dvcp import autograd
    xyz1, xyz2 = c["xyz1"].to(cuda), c["xyz2"].to(cuda)
    p1 = None if c["p1"] is None else c["p1"].detach().to(cuda).requires_grad_()
    p2 = c["p2"].detach().to(cuda).requires_grad_()
    if lin is None:
        out = mine(xyz1, xyz2, p1, p2).permute(0, 2, 1)
    else:
        out = autograd.feature_propagation(mine, xyz1, xyz2, p1, p2.permute(0, 2, 1).contiguous(), fc=lin)
    assert out.requires_grad
    (out * c["G"].to(cuda)).sum().backward()
    grads = {}
    for i, (conv, bn) in enumerate(zip(mine.mlp_convs, mine.mlp_bns)):
        grads.update({f"{i}.conv.w": conv.weight.grad, f"{i}.conv.b": conv.bias.grad, f"{i}.bn.w": bn.weight.grad,
                      f"{i}.bn.b": bn.bias.grad})
    if lin is not None:
        grads.update({"fc.w": lin.weight.grad, "fc.b": lin.bias.grad})
    if p1 is not None:
        grads["p1"] = p1.grad
    grads["p2"] = p2.grad
    assert all(v is not None and torch.isfinite(v).all() for v in grads.values())
    return out.detach(), grads


def _fp_compare(c, cuda, what):
    from dvcp import batchnorm, ops
    mine, lin = _fp_mine(c, cuda)
    out, grads = _fp_run(c, mine, lin, cuda)
    near = c["near"]
    print(f"{what}: rows left out of d points1 (a ReLU pre-activation within 1e-5 of zero) {int(near.sum())} of "
          f"{near.numel()} ({100.0 * float(near.sum()) / near.numel():.3f} %)")
    torch.testing.assert_close(out.cpu(), c["out"], rtol=1e-4, atol=1e-4)
    _buffers_close(mine, c["ref"], what)
    assert set(grads) == set(c["grads"])
    errs, bound = {}, {}
    for k in grads:
        got, want, floor = grads[k], c["grads"][k], 1e-30
        bound[k] = 1e-3
        if k.endswith("conv.b"):       # under a BN layer: true gradient zero, at the weight gradient's scale
            floor, bound[k] = float(c["grads"][k[:-1] + "w"].abs().max()), 5e-2
        if c["term"] is not None and k.endswith("conv.w"):
            assert float(want.abs().max()) < 1e-3 * c["term"], (k, float(want.abs().max()), c["term"])
            floor = c["term"]
        if k == "p1":                  # near-zero rows are left out here only; they stay in every sum
            keep = ~near
            got, want = got.permute(0, 2, 1).cpu()[keep], want.permute(0, 2, 1)[keep]
        errs[k] = _rel(got, want, floor)
    _check(what, errs, bound)
    # a second module in the same starting state: identical bits, running statistics included
    twin, lin2 = _fp_mine(c, cuda)
    out2, grads2 = _fp_run(c, twin, lin2, cuda)
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    assert all(torch.equal(a, b) for a, b in zip(mine.buffers(), twin.buffers()))
    # the raw passes: mode sums against the checker's hooks; null grad_p1 / grad_p2 leave the other bits alone
    raw, _ = _fp_mine(c, cuda)
    x1, x2 = c["xyz1"].to(cuda), c["xyz2"].to(cuda)
    p1 = None if c["p1"] is None else c["p1"].detach().to(cuda)
    p2r = c["p2"].detach().to(cuda).permute(0, 2, 1).contiguous()
    rows, st = batchnorm.fp_train_forward(raw, x1, x2, p1, p2r, lin)
    assert torch.equal(rows, out)
    g = c["G"].to(cuda)
    bn, M, chans = st["bnstat"].clone(), st["M"], st["chans"]
    so = [4 * sum(chans[1:l]) for l in range(1, len(chans))]
    serr = {}
    for k in range(st["nbn"], 0, -1):
        s = ops.feature_propagation_bn_backward(x1, x2, p2r, p1, chans, st["relu"], st["pack"], bn, g, k)
        bn[so[k - 1] + 2 * chans[k]:so[k - 1] + 4 * chans[k]] = (s / M).reshape(-1)
        # (every xhat is 0 where every row is the same row: B is then a true zero, taken at A's scale)
        bfloor = float(c["sums"][k - 1][0].abs().max()) if c["term"] is not None else 1e-30
        serr[f"A{k}"], serr[f"B{k}"] = _rel(s[0], c["sums"][k - 1][0]), _rel(s[1], c["sums"][k - 1][1], bfloor)
    _check(what + " mode sums", serr, 1e-4)
    full = ops.feature_propagation_bn_backward(x1, x2, p2r, p1, chans, st["relu"], st["pack"], bn, g, 0)
    bare = ops.feature_propagation_bn_backward(x1, x2, p2r, p1, chans, st["relu"], st["pack"], bn, g, 0,
                                               want_p1=False, want_p2=False)
    assert bare[1] is None and bare[2] is None and torch.equal(full[0], bare[0])


@pytest.mark.parametrize("B,N1", [(1, 2), (2, 31), (2, 32), (2, 33)])
@pytest.mark.parametrize("table", range(len(FP_TABLES)))
def test_feature_propagation_bn_train_vs_oracle(cuda, table, B, N1):
    """The forward test's four modules (the last one with N2 = 1) under batch statistics.  (1, 2) is M = 2,
    where biased and unbiased variance differ by a factor of 2; (2, 31 / 32 / 33): one tile per cloud,
    exactly one, one and a row."""
    N2, D1, D2, mlp = FP_TABLES[table]
    _fp_compare(_fp_case(N2, D1, D2, mlp, N1, B=B), cuda, f"fp bn train N2={N2} D1={D1} D2={D2} mlp={list(mlp)} B={B} N1={N1}")


def test_feature_propagation_bn_train_many_tiles(cuda):
    """N1 = 8193 at B = 1: 257 tiles over 256 workgroups (the first walks two), 1024 partial rows in the fold."""
    _fp_compare(_fp_case(700, 32, 64, (32, 32), 8193, B=1), cuda, "fp bn train N1=8193")


def test_feature_propagation_bn_train_fused_fc_and_coincident(cuda):
    """The extractor's last propagation (32-32-32 with the fc fused as a plain fourth layer: no statistics,
    no mean terms), and xyz2 = every fourth point of xyz1 as between the extractor's levels."""
    _fp_compare(_fp_case(700, 3, 32, (32, 32, 32), 65, fc=True), cuda, "fp bn train with fc")
    _fp_compare(_fp_case(33, 32, 64, (32, 32), 130, coincident=True), cuda, "fp bn train, coincident points")


def test_feature_propagation_bn_train_edges(cuda, monkeypatch):
    """M = 1 raises torch's ValueError with no entry point called; N2 = 2 raises as the forward does; B = 0;
    eval mode with the flag is the eval path's bits; without the flag .train() is refused."""
    import dvcp
    from dvcp import _lib, batchnorm, ops
    mine = dvcp.paper.PointNetFeaturePropagation(35, [32, 32], bn_train=True).to(cuda).train()
    calls = []
    real = _lib.call
    monkeypatch.setattr(ops, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    one = torch.zeros(1, 3, 1, device=cuda)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        mine(one, torch.zeros(1, 3, 4, device=cuda), torch.zeros(1, 3, 1, device=cuda), torch.zeros(1, 32, 4, device=cuda))
    assert calls == [] and int(mine.mlp_bns[0].num_batches_tracked) == 0
    monkeypatch.undo()
    x1, x2 = torch.rand(2, 3, 5, device=cuda), torch.rand(2, 3, 2, device=cuda)
    with pytest.raises(RuntimeError, match="N2 = 2"):
        mine(x1, x2, torch.rand(2, 3, 5, device=cuda), torch.rand(2, 32, 2, device=cuda))
    # B = 0: empty rows, zero sums and gradients, nothing updated
    e1, e2 = torch.zeros(0, 3, 5, device=cuda), torch.zeros(0, 3, 4, device=cuda)
    p1, p2r = torch.zeros(0, 3, 5, device=cuda), torch.zeros(0, 4, 32, device=cuda)
    before = int(mine.mlp_bns[0].num_batches_tracked)
    rows, st = batchnorm.fp_train_forward(mine, e1, e2, p1, p2r)
    assert rows.shape == (0, 5, 32) and int(mine.mlp_bns[0].num_batches_tracked) == before
    s = ops.feature_propagation_bn_stats(e1, e2, p2r, p1, st["chans"], st["relu"], st["pack"], 2)
    assert s.shape == (2, 32) and float(s.abs().max()) == 0.0
    gp, gp1, gp2 = batchnorm.fp_train_backward(st, e1, e2, p1, p2r, torch.zeros(0, 5, 32, device=cuda))
    assert float(gp.abs().max()) == 0.0 and gp1.shape == (0, 5, 3) and gp2.shape == (0, 4, 32)
    # eval mode: the eval path's bits, nothing updated
    plain = dvcp.paper.PointNetFeaturePropagation(35, [32, 32]).to(cuda).eval()
    plain.load_state_dict(mine.state_dict())
    a = (torch.rand(2, 3, 40, device=cuda), torch.rand(2, 3, 9, device=cuda), torch.rand(2, 3, 40, device=cuda),
         torch.rand(2, 32, 9, device=cuda))
    with torch.no_grad():
        assert torch.equal(mine.eval()(*a), plain(*a))
    assert list(plain.state_dict()) == list(mine.state_dict())
    with pytest.raises(NotImplementedError, match="PointNetFeaturePropagation.forward in training mode"):
        plain.train()(*a)


# ----------------------------------------------------------------------------------- extractor
def _condition_fe(fe, fe_scale=300.0):
    """test_gpu_paper_train.py::_condition's extractor part: the first convolution scaled."""
    with torch.no_grad():
        fe.sa1.mlp_convs[0].weight *= fe_scale


def _zero_bias(name, ref_p):
    """Floor and bar of a parameter gradient: a conv / linear bias under a BN layer has a true gradient
    of zero and is compared at its weight gradient's scale with 5e-2."""
    if name.endswith(".bias") and (".mlp_convs." in name or name.endswith(("WL.fc1.bias", "WL.fc2.bias"))):
        return float(ref_p[name[:-4] + "weight"].grad.abs().max()), 5e-2
    return 1e-30, 1e-3


@pytest.mark.parametrize("use_normal", [False, True])
def test_paper_extractor_bn_train_vs_oracle(cuda, use_normal):
    """PaperFeatExtraction(bn_train=True).train() at test_paper_extractor_backward_vs_oracle's sizes:
    features, every parameter gradient, every BN buffer after the call; a second call moves the buffers
    again; under no_grad the features are the same bits and the buffers are updated."""
    from oracle import paper as OP
    import oracle as O
    import dvcp
    from dvcp.synthetic import make_pairs
    B, N = 2, 512
    src, _, _, _ = make_pairs(B, N, normals=use_normal, seed=61)
    src = src.float()
    cfg = dict(npoints=(128, 32, 8))
    torch.manual_seed(6)
    ref = OP.PaperFeatExtraction(use_normal, **cfg)
    _randomize_bn(ref)
    _condition_fe(ref)
    ref.train()
    mine = dvcp.paper.PaperFeatExtraction(use_normal, bn_train=True, **cfg)
    mine.load_state_dict(ref.state_dict())
    mine.to(cuda).train()
    assert all(fp.bn_train for fp in (mine.fp1, mine.fp2, mine.fp3))
    starts = mine.draw_starts(B, N)
    g = torch.Generator().manual_seed(77)
    G = torch.randn(B, N, 32, generator=g)
    with O.fps_starts(list(starts)):
        want = ref(src)
    (want * G).sum().backward()
    got = mine(src.to(cuda), starts)
    assert got.requires_grad and got.shape == (B, N, 32)
    print(f"features: max |diff| {float((got.detach().cpu() - want.detach()).abs().max()):.1e}")
    torch.testing.assert_close(got.detach().cpu(), want.detach(), rtol=1e-4, atol=1e-4)
    _buffers_close(mine, ref, f"extractor use_normal={use_normal}, one call")
    (got * G.to(cuda)).sum().backward()
    errs, bound, mine_p, ref_p = {}, {}, dict(mine.named_parameters()), dict(ref.named_parameters())
    for name, p in ref_p.items():
        assert mine_p[name].grad is not None and torch.isfinite(mine_p[name].grad).all(), name
        floor, bound[name] = _zero_bias(name, ref_p)
        errs[name] = _rel(mine_p[name].grad, p.grad, floor)
    assert float(ref.sa1.mlp_convs[0].weight.grad.abs().max()) > 1e-5
    _check(f"paper extractor bn train use_normal={use_normal}", errs, bound)
    # under no_grad: the recorded forward's bits, and the buffers move again, as the checker's do
    with torch.no_grad():
        plain = mine(src.to(cuda), starts)
        with O.fps_starts(list(starts)):
            ref(src)
    assert not plain.requires_grad and torch.equal(got.detach(), plain)
    _buffers_close(mine, ref, f"extractor use_normal={use_normal}, two calls")
    assert int(mine.fp1.mlp_bns[2].num_batches_tracked) == int(mine.sa1.mlp_bns[0].num_batches_tracked) == 2
    # eval mode: the inference path's bits for the same state_dict
    off = dvcp.paper.PaperFeatExtraction(use_normal, **cfg).to(cuda).eval()
    off.load_state_dict(mine.state_dict())
    with torch.no_grad():
        assert torch.equal(mine.eval()(src.to(cuda), starts), off(src.to(cuda), starts))
    with pytest.raises(NotImplementedError, match="PaperFeatExtraction.forward in training mode"):
        off.train()(src.to(cuda), starts)


# ---------------------------------------------------------------------------------- whole step
CFG = dict(K=8, r=0.4, s=0.4, s_z=0.25, d=1.0, npoints=(128, 32, 8))   # test_gpu_paper_train.py's
SEED = 90   # chosen on the CPU: the conditions _checker_run asserts hold for this pair of pairs


def _checker_forward(ref, src, tgt, R_init, t_init):
    """test_gpu_paper_train.py's: oracle/paper.py DeepVCPPaper.forward, statement for statement, for a
    forward that records autograd (the numpy pose solve takes ``vcp`` and ``w`` detached)."""
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


def _near_tie_mask(ref, xyz, feat, S, radius, ns, start, rel=1e-5):
    """test_gpu_train.py's helper under batch statistics (``ref``: a deep copy in double, train mode)."""
    import oracle as O
    with torch.no_grad(), O.fps_starts([start]):
        _, grouped, gidx = O.sample_and_group(S, radius, ns, xyz.permute(0, 2, 1),
                                              None if feat is None else feat.permute(0, 2, 1), returnidx=True)
        x = grouped.permute(0, 3, 2, 1)
        for conv, bn in zip(ref.mlp_convs, ref.mlp_bns):
            x = torch.relu(bn(conv(x.double())))
        mx, am = x.max(2)
        pid = gidx.permute(0, 2, 1)
        pid_am = torch.gather(pid.unsqueeze(1).expand(-1, x.shape[1], -1, -1), 2, am.unsqueeze(2))
        other = torch.where(pid.unsqueeze(1) != pid_am, x, torch.full_like(x, -1.0)).max(2).values
        return (mx > 0) & (mx - other <= rel * mx)


def _condition(ref, features, fe_scale=300.0, wl_scale=10.0, target_std=2.0, cpg_scale=30.0):
    """test_gpu_paper_train.py's conditioning of the default init, the weighting layers' logits evaluated
    under batch statistics (the mode they run in here)."""
    Fn = torch.nn.functional
    with torch.no_grad():
        ref.FE.sa1.mlp_convs[0].weight *= fe_scale
        feats = features()
        for st in ref.stages:
            st.cpg.conv1.weight *= cpg_scale
            st.cpg.conv3.weight *= cpg_scale
            wl = st.WL
            wl.fc1.weight *= wl_scale
            wl.fc2.weight *= wl_scale
            h = torch.relu(Fn.batch_norm(wl.fc1(feats), None, None, wl.bn1.weight, wl.bn1.bias, True, 0.0, wl.bn1.eps))
            h = torch.relu(Fn.batch_norm(wl.fc2(h), None, None, wl.bn2.weight, wl.bn2.bias, True, 0.0, wl.bn2.eps))
            z = h @ wl.fc3.weight.t()
            scale = target_std / float(z.std())
            wl.fc3.weight *= scale
            wl.fc3.bias.fill_(-float(z.mean()) * scale)


def _checker_run(state, src, tgt, R_gt, t_gt, starts, check):
    """One step of the checker in train mode from ``state``: (model after the step, outputs, loss).
    ``check``: assert the conditions under which the two fp32 pipelines can be compared."""
    from oracle import paper as OP
    import oracle as O
    B, K = src.shape[0], CFG["K"]
    ref = OP.DeepVCPPaper(use_normal=False, **CFG)
    ref.load_state_dict(state)
    ref.train()
    order = list(starts[0]) + list(starts[1])
    fps = (ref.FE.fp3, ref.FE.fp2, ref.FE.fp1)
    pre, sa_io, handles = [], [], []
    for bn in [bn for fp in fps for bn in fp.mlp_bns] + [bn for st in ref.stages for bn in (st.WL.bn1, st.WL.bn2)]:
        handles.append(bn.register_forward_hook(lambda mod, i, o: pre.append(o.detach())))

    def sa_hook(mod, inputs, output):
        output[1].retain_grad()
        sa_io.append((copy.deepcopy(mod), inputs[0].detach(), None if inputs[1] is None else inputs[1].detach(),
                      output[1]))

    if check:
        handles += [sa.register_forward_hook(sa_hook) for sa in (ref.FE.sa1, ref.FE.sa2, ref.FE.sa3)]
    with O.fps_starts(order):
        want = _checker_forward(ref, src, tgt, R_gt, torch.zeros(1, 3))
    for h in handles:
        h.remove()
    loss = 0.0
    for si, st in enumerate(want):
        for b in range(B):
            x = st["keypts"][b].double().T.numpy()
            y = st["vcp"][b].detach().double().T.numpy()
            R1, t1 = OP.weighted_rigid_transform(x, y, st["weights"][b].detach().double().numpy())
            res = np.sort(np.linalg.norm(R1 @ x + t1[:, None] - y, axis=0))
            m = int(0.8 * K)
            gap = (res[m] - res[m - 1]) / res[m]
            if check:
                print(f"stage {si} pair {b}: rejection gap {gap:.2e} of the first dropped residual {res[m]:.2e}")
                assert gap > 1e-6 and res[m] > 1e-3, (si, b, gap, res[m])
        l, _, _ = OP.deepvcp_loss_paper_torch(st["keypts"].double().permute(0, 2, 1), st["vcp"].double().permute(0, 2, 1),
                                              st["weights"].double(), R_gt, t_gt.reshape(B, 3), 0.5, inlier_ratio=0.8)
        loss = loss + l
    loss.backward()
    if check:
        margin = min(float(a.abs().min()) for a in pre)
        print(f"smallest |ReLU pre-activation| of the propagation and weighting layers {margin:.1e}")
        assert margin > 1e-6, f"a ReLU pre-activation within {margin:.1e} of zero; choose another seed"
        assert len(sa_io) == 6
        for k, (sa, xyz, feat, out) in enumerate(sa_io):           # src sa1-3, then tgt sa1-3
            near = _near_tie_mask(sa.double().train(), xyz.double(), None if feat is None else feat.double(),
                                  sa.npoint, sa.radius, sa.nsample, starts[k // 3][k % 3])
            bad = int((near & (out.grad != 0)).sum())
            assert bad == 0, f"SA call {k}: {bad} arg-max near ties carry a gradient; choose another seed"
    return ref, want, loss.detach()


@functools.lru_cache(maxsize=None)
def _step_case():
    """The checker's whole step in train mode at B = 2 (the statistics span the pairs), the same step
    with the batch rows in the other order (the fp32 checker's own spread per tensor), and the state
    before it."""
    from oracle import paper as OP
    import oracle as O
    import dvcp
    from dvcp.synthetic import make_pairs
    B, N = 2, 512
    src, tgt, R_gt, t_gt = make_pairs(B, N, seed=SEED)
    torch.manual_seed(8)
    ref0 = OP.DeepVCPPaper(use_normal=False, **CFG)
    _randomize_bn(ref0)
    ref0.train()
    fe = dvcp.paper.PaperFeatExtraction(False, npoints=CFG["npoints"])
    starts = torch.stack([fe.draw_starts(B, N), fe.draw_starts(B, N)])

    def features():
        probe = copy.deepcopy(ref0)
        with O.fps_starts(list(starts[0])):
            return probe.FE(src).reshape(-1, 32)

    _condition(ref0, features)
    state = copy.deepcopy(ref0.state_dict())
    ref, want, loss = _checker_run(state, src, tgt, R_gt, t_gt, starts, check=True)
    flip = [1, 0]
    ref2, _, loss2 = _checker_run(state, src[flip], tgt[flip], R_gt[flip] if R_gt.shape[0] == B else R_gt,
                                  t_gt[flip] if t_gt.shape[0] == B else t_gt, starts[:, :, flip], check=False)
    spread = {n: _rel(q.grad, p.grad) for (n, p), (_, q) in zip(ref.named_parameters(), ref2.named_parameters())}
    return dict(state=state, ref=ref, want=want, loss=loss, spread=spread, src=src, tgt=tgt, R_gt=R_gt, t_gt=t_gt,
                starts=starts)


def _mine(c, cuda, **flags):
    import dvcp
    mine = dvcp.paper.DeepVCPPaper(use_normal=False, bn_train=True, **flags, **CFG)
    mine.load_state_dict(c["state"])
    return mine.to(cuda).train()


def _run(c, mine, cuda):
    import dvcp
    got = mine(c["src"].to(cuda), c["tgt"].to(cuda), c["R_gt"].to(cuda), torch.zeros(1, 3), starts=c["starts"],
               keypoint_idx=[st["topk"] for st in c["want"]])
    loss = 0.0
    for st in got:
        loss = loss + dvcp.paper.deepVCP_loss_paper(st["keypts"], st["vcp"], st["weights"], c["R_gt"].to(cuda),
                                                    c["t_gt"].to(cuda), 0.5, inlier_ratio=0.8)[0]
    return got, loss


def test_paper_bn_train_step_vs_oracle(cuda):
    """DeepVCPPaper(train_extractor=True, bn_train=True).train(): the whole step against the checker's in
    train mode, B = 2, from the checker's key points: loss, every parameter gradient, every BN buffer
    after the step (the extractor's updated twice, source then target; each WL's once), then one Adam
    step and a second forward."""
    c = _step_case()
    ref = c["ref"]
    mine = _mine(c, cuda, train_extractor=True)
    got, loss = _run(c, mine, cuda)
    for st in got:
        assert st["vcp"].requires_grad and st["weights"].requires_grad and not st["keypts"].requires_grad
        assert torch.equal(st["weights"].detach(), torch.gather(st["score"], 1, st["topk"]))
    loss.backward()
    print(f"loss {float(loss.detach()):.6f} (checker {float(c['loss']):.6f})")
    errs, scale, bound = {}, {}, {}
    mine_p, ref_p = dict(mine.named_parameters()), dict(ref.named_parameters())
    for name, p in ref_p.items():
        assert p.grad is not None and mine_p[name].grad is not None, name
        assert torch.isfinite(mine_p[name].grad).all(), name
        zero = name.endswith("cpg.conv3.bias") or (".DFE." in name and name.endswith(".bias"))
        floor, bound[name] = _zero_bias(name, ref_p)
        if zero:
            floor = 1e-3
        errs[name] = _rel(mine_p[name].grad, p.grad, floor)
        scale[name] = float(p.grad.abs().max())
        if zero:
            assert scale[name] < 1e-6, (name, scale[name])
        if bound[name] == 1e-3 and not zero and errs[name] > 1e-3:   # the issue's spread rule, for a tensor that misses 1e-3
            bound[name] = max(1e-3, min(4.0 * c["spread"][name], 5e-3))
            print(f"{name}: {errs[name]:.1e} above 1e-3; the checker's own spread {c['spread'][name]:.1e}, "
                  f"bar {bound[name]:.1e}")
    print("checker's own spread (batch rows reordered), largest:",
          {k: f"{v:.1e}" for k, v in sorted(c["spread"].items(), key=lambda kv: -kv[1])[:6]})
    torch.testing.assert_close(loss.detach().cpu(), c["loss"], rtol=1e-4, atol=0)
    assert scale["FE.sa1.mlp_convs.0.weight"] > 1e-5 and scale["FE.fp1.mlp_convs.0.weight"] > 1e-5   # not vacuous
    _check("paper bn train step", errs, bound)
    _buffers_close(mine, ref, "after the step")
    assert int(mine.FE.sa1.mlp_bns[0].num_batches_tracked) == int(mine.FE.fp1.mlp_bns[2].num_batches_tracked) == 2
    assert all(int(st.WL.bn1.num_batches_tracked) == int(st.WL.bn2.num_batches_tracked) == 1 for st in mine.stages)
    opt = torch.optim.Adam([p for p in mine.parameters() if p.requires_grad], lr=1e-3)
    before = mine_p["FE.fp1.mlp_convs.0.weight"].detach().clone()
    opt.step()
    assert not torch.equal(before, mine_p["FE.fp1.mlp_convs.0.weight"].detach())
    _, loss2 = _run(c, mine, cuda)
    assert torch.isfinite(loss2)


def test_paper_bn_train_frozen_extractor_and_eval(cuda):
    """train_heads=True, bn_train=True in train mode with a frozen extractor: the extractor's buffers move
    (twice per step), no extractor parameter gets a gradient; then .eval() gives the inference path's bits
    for the same state_dict."""
    import dvcp
    c = _step_case()
    mine = _mine(c, cuda, train_heads=True)
    mine.FE.requires_grad_(False)
    before = copy.deepcopy(mine.FE.state_dict())
    _, loss = _run(c, mine, cuda)
    loss.backward()
    assert all(p.grad is None for p in mine.FE.parameters())
    assert all(p.grad is not None for p in mine.stages.parameters())
    for k, v in mine.FE.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 2, k
        elif "running" in k:
            assert not torch.equal(v, before[k]), k
    _buffers_close(mine, c["ref"], "frozen extractor, after the step")
    plain = dvcp.paper.DeepVCPPaper(use_normal=False, **CFG).to(cuda).eval()
    plain.load_state_dict(mine.state_dict())
    args = (c["src"].to(cuda), c["tgt"].to(cuda), c["R_gt"].to(cuda), torch.zeros(1, 3))
    with torch.no_grad():
        a, b = mine.eval()(*args, starts=c["starts"]), plain(*args, starts=c["starts"])
    for x, y in zip(a, b):
        for k in ("vcp", "weights", "R", "t", "keypts", "score", "topk"):
            assert torch.equal(x[k], y[k]), k
