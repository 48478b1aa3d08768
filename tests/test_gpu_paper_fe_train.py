"""Paper mode, training of the extractor (dvcp.paper with autograd): the feature-propagation backward
(dvcp_feature_propagation_backward) and the group-rows backward (dvcp_group_rows_backward; both
csrc/paper_fe_bwd.hip), the paper's sa1 tables in dvcp_sa_group_mlp_backward, then
PaperFeatExtraction and DeepVCPPaper(train_extractor=True), against torch autograd through the
checker's modules (oracle/paper.py) in fp32 -- the dtype in which the forward tests match it (its
modules cast .float() inside, and the 3-NN weights at coincident points are decided by fp32 rounding).

Bars.  Kernel tests: 1e-4 of each tensor's maximum (test_sa_backward_vs_oracle's bar), group rows 1e-5
(the sums differ only in order).  Extractor and whole step: 1e-3 of each tensor's maximum
(test_fe_train_step_vs_oracle's), loss rtol 1e-4, head gradients as test_gpu_paper_train.py.

Rows of the propagation MLP are independent.  A row with a ReLU pre-activation of the fp32 checker
within 1e-5 of zero may be masked differently by the two fp32 pipelines, so it gets a zero output
gradient on both sides; their number is printed and at most 1 % of the rows (the seeds were chosen on
the CPU for that).  The backward runs min(tiles, 256) workgroups over tiles of 32 rows: N1 = 1, 31,
32, 33 are around one tile, N1 = 8193 at B = 1 gives 257 tiles (one workgroup walks two)."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FP_SEED = 3000   # chosen on the CPU: every case below zeroes at most 1 % of its rows
FP_TABLES = [(700, 32, 64, (32, 32)), (700, 0, 32, (32, 32, 32)), (3, 64, 64, (64, 64)), (1, 0, 32, (16,))]


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


def _bn_outputs(modules):
    """Forward hooks that collect every BatchNorm output (the ReLU pre-activations) of ``modules``."""
    got, handles = [], []
    for m in modules:
        handles.append(m.register_forward_hook(lambda mod, i, o: got.append(o.detach())))
    return got, handles


# ------------------------------------------------------------------------- feature propagation
@functools.lru_cache(maxsize=None)
def _fp_case(N2, D1, D2, mlp, N1, B=2, fc=False, coincident=False):
    """One fp32 checker run (forward, near-zero rows, backward), shared by the tests and read-only."""
    from oracle import paper as OP
    g = torch.Generator().manual_seed(FP_SEED + 7 * N2 + D1 + 13 * N1)
    torch.manual_seed(5)
    ref = OP.PointNetFeaturePropagation(D1 + D2, list(mlp)).eval()
    _randomize_bn(ref)
    lin = torch.nn.Linear(mlp[-1], 32) if fc else None
    xyz1 = torch.rand(B, 3, N1, generator=g) * 2 - 1
    if coincident:   # xyz2 = every fourth point of xyz1, as in the extractor (d = 0 up to rounding)
        xyz2 = xyz1[:, :, ::4].contiguous()
        assert xyz2.shape[2] == N2
    else:
        xyz2 = torch.rand(B, 3, N2, generator=g) * 2 - 1
    p1 = torch.randn(B, D1, N1, generator=g).requires_grad_() if D1 else None
    p2 = torch.randn(B, D2, N2, generator=g).requires_grad_()
    pre, handles = _bn_outputs(ref.mlp_bns)
    out = ref(xyz1, xyz2, p1, p2).permute(0, 2, 1)              # (B, N1, C) rows
    for h in handles:
        h.remove()
    if lin is not None:
        out = lin(out)
    near = torch.zeros(B, N1, dtype=torch.bool)
    for a in pre:                                               # (B, C, N1)
        near |= (a.abs() < 1e-5).any(1)
    G = torch.randn(out.shape, generator=g)
    G[near] = 0.0
    (out * G).sum().backward()
    grads = {}
    for i, (conv, bn) in enumerate(zip(ref.mlp_convs, ref.mlp_bns)):
        grads.update({f"{i}.conv.w": conv.weight.grad, f"{i}.conv.b": conv.bias.grad, f"{i}.bn.w": bn.weight.grad,
                      f"{i}.bn.b": bn.bias.grad})
    if lin is not None:
        grads.update({"fc.w": lin.weight.grad, "fc.b": lin.bias.grad})
    if p1 is not None:
        grads["p1"] = p1.grad
    grads["p2"] = p2.grad
    return dict(ref=ref, lin=lin, xyz1=xyz1, xyz2=xyz2, p1=p1, p2=p2, out=out.detach(), G=G, grads=grads,
                zeroed=int(near.sum()), rows=B * N1)


def _fp_mine(c, cuda):
    import dvcp
    ref = c["ref"]
    mine = dvcp.paper.PointNetFeaturePropagation(ref.mlp_convs[0].in_channels,
                                                 [conv.out_channels for conv in ref.mlp_convs]).eval()
    mine.load_state_dict(ref.state_dict())
    lin = None if c["lin"] is None else copy.deepcopy(c["lin"]).to(cuda)
    if lin is not None:
        lin.zero_grad()
    return mine.to(cuda), lin


def _fp_run(c, mine, lin, cuda):
    """The module (or, with a fused fc, autograd.feature_propagation) recorded and backpropagated:
    -> (out rows, {name: gradient})."""
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
    mine, lin = _fp_mine(c, cuda)
    out, grads = _fp_run(c, mine, lin, cuda)
    print(f"{what}: rows zeroed (a ReLU pre-activation within 1e-5 of zero) {c['zeroed']} of {c['rows']}")
    assert c["zeroed"] <= 0.01 * c["rows"], "choose another seed"
    torch.testing.assert_close(out.cpu(), c["out"], rtol=1e-5, atol=1e-5)
    assert set(grads) == set(c["grads"])
    _check(what, {k: _rel(grads[k], c["grads"][k]) for k in grads}, 1e-4)
    # the recorded forward is the inference kernel: the same bits
    with torch.no_grad():
        if lin is None:
            plain = mine(c["xyz1"].to(cuda), c["xyz2"].to(cuda), None if c["p1"] is None else c["p1"].detach().to(cuda),
                         c["p2"].detach().to(cuda)).permute(0, 2, 1)
        else:
            plain = mine.run(c["xyz1"].to(cuda), c["xyz2"].to(cuda),
                             None if c["p1"] is None else c["p1"].detach().to(cuda),
                             c["p2"].detach().to(cuda).permute(0, 2, 1).contiguous(), fc=lin)
    assert not plain.requires_grad and torch.equal(out, plain)
    assert all(bn.running_mean.grad is None for bn in mine.mlp_bns)


@pytest.mark.parametrize("N1", [1, 31, 32, 33])
@pytest.mark.parametrize("table", range(len(FP_TABLES)))
def test_feature_propagation_backward_vs_oracle(cuda, table, N1):
    """Every dW, db, dgamma, dbeta, d points1 and d points2 of the forward test's four modules against
    the checker's autograd via (out * G).sum().backward(), around the 32-row tile, B = 2."""
    N2, D1, D2, mlp = FP_TABLES[table]
    _fp_compare(_fp_case(N2, D1, D2, mlp, N1), cuda, f"fp backward N2={N2} D1={D1} D2={D2} mlp={list(mlp)} N1={N1}")


def test_feature_propagation_backward_many_tiles(cuda):
    """N1 = 8193 at B = 1: 257 tiles over 256 workgroups, the last tile one row; 700 interpolation
    points (one LDS tile of xyz2) and 1100 (two)."""
    for N2 in (700, 1100):
        _fp_compare(_fp_case(N2, 32, 64, (32, 32), 8193, B=1), cuda, f"fp backward N1=8193 N2={N2}")


def test_feature_propagation_backward_fused_fc(cuda):
    """The extractor's last propagation: 32-32-32 with the fc fused as a fourth layer (no BN, no ReLU)."""
    _fp_compare(_fp_case(700, 0, 32, (32, 32, 32), 33, fc=True), cuda, "fp backward with fc")
    _fp_compare(_fp_case(700, 3, 32, (32, 32, 32), 65, fc=True), cuda, "fp backward with fc, normals")


def test_feature_propagation_backward_coincident_points(cuda):
    """xyz2 = every fourth point of xyz1, as between the extractor's levels: a quarter of the rows has
    its nearest neighbour at d = 0 up to the expansion form's rounding."""
    _fp_compare(_fp_case(33, 32, 64, (32, 32), 130, coincident=True), cuda, "fp backward, coincident points")


@pytest.mark.parametrize("N2,coincident", [(3, False), (1, False), (30, False), (9, True)])
def test_three_nn_indices_exact(cuda, N2, coincident):
    """The neighbours are the checker's, exactly: with points2 = [I, -I] (one-hot rows and their
    negatives) and a layer that is the identity (W = I, b = 0, BN with mean 0, var 1 - eps, weight 1,
    bias 0) the output row holds relu(w) and relu(-w) of the three interpolation weights at the
    neighbours' indices; a weight at a coincident point may come out negative on either side (d is
    0 up to the expansion form's rounding, and 1 / (d + 1e-8) changes sign below -1e-8), hence both
    signs.  The same non-zero pattern on both sides; the values within the forward test's bar
    (test_gpu_paper.py::test_feature_propagation_vs_oracle: the two far neighbours of a coincident
    point weigh (d + 1e-8) / d_i, a few 1e-6 of either sign)."""
    from oracle import paper as OP
    import dvcp
    g = torch.Generator().manual_seed(40 + N2)
    B, N1, C = 2, 33, 2 * N2
    ref = OP.PointNetFeaturePropagation(C, [C]).eval()
    with torch.no_grad():
        ref.mlp_convs[0].weight.copy_(torch.eye(C)[:, :, None])
        ref.mlp_convs[0].bias.zero_()
        ref.mlp_bns[0].running_var.fill_(1.0 - ref.mlp_bns[0].eps)
    mine = dvcp.paper.PointNetFeaturePropagation(C, [C]).eval()
    mine.load_state_dict(ref.state_dict())
    mine.to(cuda)
    xyz1 = torch.rand(B, 3, N1, generator=g) * 2 - 1
    xyz2 = xyz1[:, :, ::4].contiguous() if coincident else torch.rand(B, 3, N2, generator=g) * 2 - 1
    assert xyz2.shape[2] == N2
    p2 = torch.cat([torch.eye(N2), -torch.eye(N2)], 0)[None].expand(B, C, N2).contiguous()
    with torch.no_grad():
        want = ref(xyz1, xyz2, None, p2)
        got = mine(xyz1.to(cuda), xyz2.to(cuda), None, p2.to(cuda)).cpu()
    pattern = lambda o: (o[:, :N2] != 0) | (o[:, N2:] != 0)   # noqa: E731  (B, N2, N1): point n uses neighbour j
    assert int(pattern(want).sum()) == B * N1 * min(N2, 3)
    assert torch.equal(pattern(got), pattern(want))
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)


def _bnstat(mine, lin=None):
    parts = []
    for bn in mine.mlp_bns:
        parts += [bn.running_mean.float(), torch.rsqrt(bn.running_var.double() + bn.eps).float()]
    if lin is not None:
        n = lin.weight.shape[0]
        parts += [torch.zeros(n, device=lin.weight.device), torch.ones(n, device=lin.weight.device)]
    return torch.cat(parts).contiguous()


def test_feature_propagation_backward_edges(cuda):
    from dvcp import ops
    import dvcp
    c = _fp_case(700, 32, 64, (32, 32), 33)
    mine, _ = _fp_mine(c, cuda)
    chans, relu, params, bnstat = mine.chans, [1, 1], mine.packed_params(), _bnstat(mine)
    xyz1, xyz2 = c["xyz1"].to(cuda), c["xyz2"].to(cuda)
    p1, p2r = c["p1"].detach().to(cuda), c["p2"].detach().to(cuda).permute(0, 2, 1).contiguous()
    G = c["G"].to(cuda)
    call = lambda **kw: ops.feature_propagation_backward(xyz1, xyz2, p2r, p1, chans, relu, params, bnstat, G, **kw)  # noqa: E731
    # two identical calls: identical bits in every output
    one, two = call(), call()
    assert all(torch.equal(a, b) for a, b in zip(one, two))
    assert _rel(one[1].permute(0, 2, 1), c["grads"]["p1"]) <= 1e-4 and _rel(one[2].permute(0, 2, 1), c["grads"]["p2"]) <= 1e-4
    # grad_p1 / grad_p2 null: the parameter gradients are the same bits
    for w1, w2 in ((False, False), (True, False), (False, True)):
        gp, g1, g2 = call(want_p1=w1, want_p2=w2)
        assert (g1 is None) == (not w1) and (g2 is None) == (not w2) and torch.equal(gp, one[0])
        assert g1 is None or torch.equal(g1, one[1])
        assert g2 is None or torch.equal(g2, one[2])
    # B = 0 and N1 = 0: zero parameter gradients (and nothing routed to points2)
    z = lambda *s: torch.zeros(*s, device=cuda)   # noqa: E731
    gp, g1, g2 = ops.feature_propagation_backward(z(0, 3, 33), z(0, 3, 700), z(0, 700, 64), z(0, 32, 33), chans, relu,
                                                  params, bnstat, z(0, 33, 32))
    assert gp.shape == (ops.fp_nparams(chans),) and float(gp.abs().max()) == 0.0 and g1.shape == (0, 33, 32)
    gp, g1, g2 = ops.feature_propagation_backward(z(2, 3, 0), xyz2, p2r, z(2, 32, 0), chans, relu, params, bnstat,
                                                  z(2, 0, 32))
    assert float(gp.abs().max()) == 0.0 and g2.shape == (2, 700, 64) and float(g2.abs().max()) == 0.0
    # N2 = 2 raises on both sides, forward and backward
    x2 = torch.rand(2, 3, 2)
    with pytest.raises(RuntimeError):
        c["ref"](c["xyz1"], x2, c["p1"].detach(), torch.randn(2, 64, 2))
    with pytest.raises(RuntimeError, match="N2 = 2"):
        mine(xyz1, x2.to(cuda), p1, torch.randn(2, 64, 2, device=cuda, requires_grad=True))
    with pytest.raises(RuntimeError, match="dvcp_feature_propagation_backward: N2 = 2"):
        ops.feature_propagation_backward(xyz1, x2.to(cuda), z(2, 2, 64), p1, chans, relu, params, bnstat, G)
    # d points2 of another width than 32 / 64 is refused; without it the call goes through
    m48 = dvcp.paper.PointNetFeaturePropagation(48, [16]).eval().to(cuda)
    a48 = (xyz1, xyz2, z(2, 700, 48), None, m48.chans, [1], m48.packed_params(), _bnstat(m48), z(2, 33, 16))
    with pytest.raises(RuntimeError, match=r"grad_p2 with D2=48 \(segment_sum takes 32 or 64 columns\)"):
        ops.feature_propagation_backward(*a48)
    assert ops.feature_propagation_backward(*a48, want_p2=False)[2] is None
    # a frozen layer with points2 requiring a gradient: only d points2
    frozen, _ = _fp_mine(c, cuda)
    frozen.requires_grad_(False)
    p2 = c["p2"].detach().to(cuda).requires_grad_()
    out = frozen(xyz1, xyz2, p1, p2)
    assert out.requires_grad
    (out.permute(0, 2, 1) * G).sum().backward()
    assert all(p.grad is None for p in frozen.parameters()) and p1.grad is None
    assert _rel(p2.grad, c["grads"]["p2"]) <= 1e-4
    # nothing requires a gradient: the inference path
    assert not frozen(xyz1, xyz2, p1, p2.detach()).requires_grad
    with pytest.raises(NotImplementedError, match="training mode"):
        mine.train()(xyz1, xyz2, p1, p2)


# ---------------------------------------------------------------------------------- group rows
@functools.lru_cache(maxsize=None)
def _group_rows_case(N, ns):
    """test_gpu_paper.py::test_group_rows_vs_oracle's inputs (generator 62, drawn in its order)."""
    from oracle import paper as OP
    g = torch.Generator().manual_seed(62)
    for n_, ns_ in ((2000, 32), (20, 32)):
        B, Q = 2, 300
        xyz = torch.rand(B, n_, 3, generator=g) * 2 - 1
        feats = torch.randn(B, n_, 32, generator=g)
        ctr = torch.rand(B, Q, 3, generator=g) * 6 - 3
        if n_ == N:
            break
    feats.requires_grad_()
    rows = OP.group_rows(ctr, xyz, feats, 0.5, ns)
    G = torch.randn(rows.shape, generator=g)
    (rows * G).sum().backward()
    return dict(xyz=xyz, feats=feats, ctr=ctr, rows=rows.detach(), G=G, gfeat=feats.grad)


@pytest.mark.parametrize("N", [2000, 20])
def test_group_rows_backward_vs_oracle(cuda, N):
    """d feat through the DFE rows' gather against the checker's autograd: N = 2000, and N = 20 with 32
    slots (above the cloud size: padding with the first hit); most centres lie far outside (empty
    neighbourhoods route nothing)."""
    from dvcp import autograd, ops
    ns = 32
    c = _group_rows_case(N, ns)
    x, ctr, G = c["xyz"].to(cuda), c["ctr"].to(cuda), c["G"].to(cuda)
    cnt, lst, _ = ops.ball_query(x, ctr, 0.5, min(ns, N), pdim=1, cdim_pts=1)
    assert bool((cnt == 0).any()) and bool((cnt > 0).any())
    one = ops.group_rows_backward(cnt, lst, ns, N, G)
    two = ops.group_rows_backward(cnt, lst, ns, N, G)
    assert one.shape == (2, N, 32) and torch.equal(one, two)           # two calls: identical bits
    _check(f"group rows backward N={N}", {"d feat": _rel(one, c["gfeat"])}, 1e-5)
    untouched = c["gfeat"].abs().sum(-1) == 0                          # points in no list
    hit = torch.zeros(2, N + 1, dtype=torch.bool, device=cuda)
    valid = torch.arange(lst.shape[2], device=cuda)[None, None] < cnt[..., None].clamp(max=lst.shape[2])
    hit.scatter_(1, torch.where(valid, lst.long(), torch.full_like(lst.long(), N)).reshape(2, -1), True)
    assert torch.equal(~hit[:, :N].cpu(), untouched)
    assert bool(untouched.any()) and bool((one.cpu()[untouched] == 0).all())
    # the autograd path: the forward bits are the inference path's (and the checker's), then the same d feat
    f = c["feats"].detach().to(cuda).requires_grad_()
    rows = autograd.group_rows(ctr, x.permute(0, 2, 1), f, cnt, lst, ns, 0.5)
    plain = ops.group_rows(ctr, x, f.detach(), cnt, lst, ns, 0.5, ctr_pdim=1, xyz_pdim=1)
    assert rows.requires_grad and torch.equal(rows.detach(), plain)
    torch.testing.assert_close(plain.cpu(), c["rows"], rtol=0, atol=0)
    (rows * G).sum().backward()
    assert torch.equal(f.grad, one)
    with pytest.raises(RuntimeError, match=r"dvcp_group_rows_backward: D=16 \(32 feature columns only\)"):
        ops.group_rows_backward(cnt, lst, ns, N, torch.zeros(2, 300, ns, 19, device=cuda))


def test_dfe_tgt_feature_grad_same_bits_small(cuda):
    """segment_sum now forwards to its strided form (stride = columns, offset 0): the packed caller's
    target-feature gradient is still the same bits in two calls (the yardstick is
    test_gpu_train.py::test_dfe_tgt_feature_grad_bit_identical) and zero where no entry lands."""
    from dvcp import ops
    import dvcp
    torch.manual_seed(13)
    B, M, Q = 2, 300, 500
    xyz = (torch.rand(B, 3, M) * 2 - 1).to(cuda)
    feat = torch.rand(B, M, 32).to(cuda)
    qry = (torch.rand(B, Q, 3) * 0.6 - 0.3).to(cuda)
    dist, idx, _ = ops.knn(xyz, qry, 32, ref_pdim=2, qry_pdim=1, want_idx64=False)
    params = dvcp.feat_embedding_layer().to(cuda).packed_params()
    g = torch.randn(B, Q, 32, device=cuda)
    one = ops.dfe_tgt_backward(xyz, feat, qry, dist, idx, params, g, want_feat_grad=True)
    two = ops.dfe_tgt_backward(xyz, feat, qry, dist, idx, params, g, want_feat_grad=True)
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
    hit = torch.zeros(B, M, dtype=torch.bool, device=cuda)
    hit.scatter_(1, idx.reshape(B, -1).long(), True)
    assert (~hit).any() and bool((one[1][~hit] == 0).all()) and float(one[1].abs().max()) > 0


# ------------------------------------------------------------------- SA backward, paper sa1 tables
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
def test_sa_backward_paper_sa1_vs_oracle(cuda, D):
    """The paper's first set abstraction (3 + D -> 32 -> 32, without / with normals) in
    dvcp_sa_group_mlp_backward, by test_sa_backward_vs_oracle's recipe: S = 128 centres, 32 slots, a
    radius at which the median neighbourhood holds at least 8 points."""
    import oracle as O
    import dvcp
    from dvcp import autograd, ops
    g = torch.Generator().manual_seed(410 + D)
    B, N, S, ns, radius = 2, 1024, 128, 32, 0.12
    xyz = torch.rand(B, 3, N, generator=g) * 0.6 - 0.3
    feat = None
    if D:
        feat = torch.randn(B, 3, N, generator=g)
        feat = feat / feat.norm(dim=1, keepdim=True)
    torch.manual_seed(11)
    ref = O.PointNetSetAbstraction(S, radius, ns, 3 + D, [32, 32]).eval()
    _randomize_bn(ref)
    mine = dvcp.pointnet2_utils.PointNetSetAbstraction(S, radius, ns, 3 + D, [32, 32]).eval()
    mine.load_state_dict(ref.state_dict())
    mine.to(cuda)
    start = torch.randint(0, N, (B,), generator=g)
    G = torch.randn(B, 32, S, generator=g)
    near = _near_tie_mask(copy.deepcopy(ref).double(), xyz.double(), None if feat is None else feat.double(), S, radius,
                          ns, start)
    G[near] = 0.0
    with O.fps_starts([start]):
        _, out_o = ref(xyz, feat)
    (out_o * G).sum().backward()
    with torch.no_grad():                                         # the neighbourhoods are filled
        ctr_o = O.index_points(xyz.permute(0, 2, 1), O.farthest_point_sample(xyz.permute(0, 2, 1), S, start=start))
    d2 = ((ctr_o[:, :, None, :] - xyz.permute(0, 2, 1)[:, None]) ** 2).sum(-1)
    median = float((d2 <= radius * radius).sum(-1).float().median())
    print(f"D={D}: median neighbourhood {median:.0f} points")
    assert median >= 8

    x, f = xyz.to(cuda), (None if feat is None else feat.to(cuda))
    _, ctr = ops.fps(x, S, start.to(cuda), pdim=2)
    count, lst, _ = ops.ball_query(x, ctr, radius, ns, pdim=2, cdim_pts=2)
    out = ops.sa_group_mlp(x, ctr, f, count, lst, ns, mine.chans, mine.packed_params(), xyz_pdim=2, feat_ddim=1,
                           feat_pdim=2)
    torch.testing.assert_close(out.permute(0, 2, 1).cpu(), out_o.detach(), rtol=1e-5, atol=1e-5)
    gp, gF = ops.sa_group_mlp_backward(x, ctr, f, count, lst, ns, mine.chans, mine.packed_params(),
                                       autograd._bn_stats(mine), G.permute(0, 2, 1).float().to(cuda),
                                       want_feat_grad=False)
    assert gF is None
    o, errs = 0, {}
    for i, (conv, bn) in enumerate(zip(ref.mlp_convs, ref.mlp_bns)):
        co, ci = conv.weight.shape[:2]
        for name, want, n in (("conv.w", conv.weight.grad.reshape(co, ci), co * ci), ("conv.b", conv.bias.grad, co),
                              ("bn.w", bn.weight.grad, co), ("bn.b", bn.bias.grad, co)):
            errs[f"{i}.{name}"] = _rel(gp[o:o + n].view(want.shape), want)
            o += n
    print(f"D={D}: near-tie pairs left out: {int(near.sum())} of {near.numel()}")
    _check(f"paper sa1 backward D={D}", errs, 1e-4)


# ----------------------------------------------------------------------------------- extractor
def _condition_fe(fe, fe_scale=300.0):
    """test_gpu_paper_train.py::_condition's extractor part: the first convolution scaled."""
    with torch.no_grad():
        fe.sa1.mlp_convs[0].weight *= fe_scale


@pytest.mark.parametrize("use_normal", [False, True])
def test_paper_extractor_backward_vs_oracle(cuda, use_normal):
    """PaperFeatExtraction with every parameter trainable: each gradient against the checker's autograd
    under the same FPS starts (1e-3 of the tensor's maximum: arg-max flips on fp32 near-ties are
    tolerated as in test_fe_train_step_vs_oracle; the kernels' own 1e-4 bars are above), the recorded
    forward torch.equal to the no_grad forward."""
    from oracle import paper as OP
    import oracle as O
    import dvcp
    from dvcp.synthetic import make_pairs
    B, N = 2, 512
    src, _, _, _ = make_pairs(B, N, normals=use_normal, seed=61)
    src = src.float()
    cfg = dict(npoints=(128, 32, 8))
    torch.manual_seed(6)
    ref = OP.PaperFeatExtraction(use_normal, **cfg).eval()
    _randomize_bn(ref)
    _condition_fe(ref)
    mine = dvcp.paper.PaperFeatExtraction(use_normal, **cfg).eval()
    mine.load_state_dict(ref.state_dict())
    mine.to(cuda)
    starts = mine.draw_starts(B, N)
    g = torch.Generator().manual_seed(77)
    G = torch.randn(B, N, 32, generator=g)
    with O.fps_starts(list(starts)):
        want = ref(src)
    (want * G).sum().backward()
    got = mine(src.to(cuda), starts)
    assert got.requires_grad and got.shape == (B, N, 32)
    with torch.no_grad():
        plain = mine(src.to(cuda), starts)
    assert not plain.requires_grad and torch.equal(got.detach(), plain)
    torch.testing.assert_close(got.detach().cpu(), want.detach(), rtol=1e-4, atol=1e-4)
    (got * G.to(cuda)).sum().backward()
    errs, mine_p = {}, dict(mine.named_parameters())
    for name, p in ref.named_parameters():
        assert mine_p[name].grad is not None and torch.isfinite(mine_p[name].grad).all(), name
        errs[name] = _rel(mine_p[name].grad, p.grad)
    assert float(ref.sa1.mlp_convs[0].weight.grad.abs().max()) > 1e-5
    assert all(b.grad is None for b in (mine.sa1.mlp_bns[0].running_mean, mine.fp1.mlp_bns[0].running_var))
    _check(f"paper extractor backward use_normal={use_normal}", errs, 1e-3)
    with pytest.raises(NotImplementedError, match="training mode"):
        mine.train()(src.to(cuda), starts)


# ---------------------------------------------------------------------------------- whole step
CFG = dict(K=8, r=0.4, s=0.4, s_z=0.25, d=1.0, npoints=(128, 32, 8))   # test_gpu_paper_train.py's


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


def _condition(ref, features, fe_scale=300.0, wl_scale=10.0, target_std=2.0, cpg_scale=30.0):
    """test_gpu_paper_train.py's conditioning of the default init (see there for the why)."""
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


SEED = 89   # chosen on the CPU: the conditions _checker_step asserts hold for this pair


@functools.lru_cache(maxsize=None)
def _pair():
    """The checker's model, inputs and FPS starts (CPU), shared and read-only apart from .grad."""
    from oracle import paper as OP
    import oracle as O
    import dvcp
    from dvcp.synthetic import make_pairs
    B, N = 1, 512
    src, tgt, R_gt, t_gt = make_pairs(B, N, seed=SEED)
    torch.manual_seed(8)
    ref = OP.DeepVCPPaper(use_normal=False, **CFG).eval()
    _randomize_bn(ref)
    fe = dvcp.paper.PaperFeatExtraction(False, npoints=CFG["npoints"])
    starts = torch.stack([fe.draw_starts(B, N), fe.draw_starts(B, N)])

    def features():
        with O.fps_starts(list(starts[0])):
            return ref.FE(src).reshape(-1, 32)

    _condition(ref, features)
    return ref, src, tgt, R_gt, t_gt, starts


def _mine(cuda, **flags):
    import dvcp
    ref = _pair()[0]
    mine = dvcp.paper.DeepVCPPaper(use_normal=False, **flags, **CFG).eval()
    mine.load_state_dict(ref.state_dict())
    return mine.to(cuda)


def _loss(mine, got, R_gt, t_gt, cuda):
    import dvcp
    loss = 0.0
    for st in got:
        loss = loss + dvcp.paper.deepVCP_loss_paper(st["keypts"], st["vcp"], st["weights"], R_gt.to(cuda), t_gt.to(cuda),
                                                    0.5, inlier_ratio=0.8)[0]
    return loss


@functools.lru_cache(maxsize=None)
def _checker_step():
    """The checker's training step with the extractor trainable, and the conditions under which the two
    fp32 pipelines can be compared (asserted here, on the CPU)."""
    from oracle import paper as OP
    import oracle as O
    ref, src, tgt, R_gt, t_gt, starts = _pair()
    B, K = 1, CFG["K"]
    ref.zero_grad()
    order = list(starts[0]) + list(starts[1])
    with torch.no_grad(), O.fps_starts(order):
        plain = ref(src, tgt, R_gt, torch.zeros(1, 3))
    fps = (ref.FE.fp3, ref.FE.fp2, ref.FE.fp1)
    sas = (ref.FE.sa1, ref.FE.sa2, ref.FE.sa3)
    pre, handles = _bn_outputs([bn for fp in fps for bn in fp.mlp_bns])
    sa_io = []

    def sa_hook(mod, inputs, output):
        output[1].retain_grad()
        sa_io.append((mod, inputs[0].detach(), None if inputs[1] is None else inputs[1].detach(), output[1]))

    handles += [sa.register_forward_hook(sa_hook) for sa in sas]
    with O.fps_starts(order):
        want = _checker_forward(ref, src, tgt, R_gt, torch.zeros(1, 3))
    for h in handles:
        h.remove()
    loss_o = 0.0
    for si, (st, pl) in enumerate(zip(want, plain)):
        assert torch.equal(st["vcp"].detach(), pl["vcp"]) and torch.equal(st["weights"].detach(), pl["weights"]), si
        assert torch.equal(st["topk"], pl["topk"]) and torch.equal(st["R"], pl["R"]), si
        # the rejection cut (6 of 8 kept) is no near tie under the first solve
        x = st["keypts"][0].double().T.numpy()
        y = st["vcp"][0].detach().double().T.numpy()
        R1, t1 = OP.weighted_rigid_transform(x, y, st["weights"][0].detach().double().numpy())
        res = np.sort(np.linalg.norm(R1 @ x + t1[:, None] - y, axis=0))
        m = int(0.8 * K)
        gap = (res[m] - res[m - 1]) / res[m]
        print(f"stage {si}: rejection gap {gap:.2e} of the first dropped residual {res[m]:.2e}")
        assert gap > 1e-6 and res[m] > 1e-3, f"stage {si}: rejection near tie ({gap:.1e}, {res[m]:.1e}); choose another seed"
        l, _, _ = OP.deepvcp_loss_paper_torch(st["keypts"].double().permute(0, 2, 1), st["vcp"].double().permute(0, 2, 1),
                                              st["weights"].double(), R_gt, t_gt.reshape(B, 3), 0.5, inlier_ratio=0.8)
        loss_o = loss_o + l
    loss_o.backward()
    margin = min(float(a.abs().min()) for a in pre)
    print(f"smallest |ReLU pre-activation| of the propagation layers {margin:.1e}")
    assert margin > 1e-6, f"a propagation ReLU pre-activation within {margin:.1e} of zero; choose another seed"
    assert len(sa_io) == 6
    for k, (sa, xyz, feat, out) in enumerate(sa_io):               # src sa1-3, then tgt sa1-3
        near = _near_tie_mask(copy.deepcopy(sa).double(), xyz.double(), None if feat is None else feat.double(),
                              sa.npoint, sa.radius, sa.nsample, starts[k // 3][k % 3])
        bad = int((near & (out.grad != 0)).sum())
        assert bad == 0, f"SA call {k}: {bad} arg-max near ties carry a gradient; choose another seed"
    return want, loss_o


def test_paper_extractor_train_step_vs_oracle(cuda):
    """DeepVCPPaper(train_extractor=True): forward, the paper loss summed over both stages, backward, one
    Adam step, against the checker's own step with the extractor trainable on both sides (B = 1,
    N = 512, K = 8; the GPU run from the checker's key points)."""
    ref, src, tgt, R_gt, t_gt, starts = _pair()
    want, loss_o = _checker_step()
    mine = _mine(cuda, train_extractor=True)

    def run():
        got = mine(src.to(cuda), tgt.to(cuda), R_gt.to(cuda), torch.zeros(1, 3), starts=starts,
                   keypoint_idx=[st["topk"] for st in want])
        return got, _loss(mine, got, R_gt, t_gt, cuda)

    got, loss = run()
    for st in got:
        assert st["vcp"].requires_grad and st["weights"].requires_grad and not st["keypts"].requires_grad
        assert torch.equal(st["weights"].detach(), torch.gather(st["score"], 1, st["topk"]))
    loss.backward()
    print(f"loss {float(loss.detach()):.6f} (checker {float(loss_o.detach()):.6f})")
    errs, scale, bound = {}, {}, {}
    mine_p = dict(mine.named_parameters())
    for name, p in ref.named_parameters():
        assert p.grad is not None and mine_p[name].grad is not None, name
        assert torch.isfinite(mine_p[name].grad).all(), name
        zero = name.endswith("cpg.conv3.bias") or (".DFE." in name and name.endswith(".bias"))
        errs[name] = _rel(mine_p[name].grad, p.grad, 1e-3 if zero else 1e-30)
        scale[name] = float(p.grad.abs().max())
        bound[name] = 1e-3
        if zero:   # floored because the true gradient is zero: the checker's own value says so
            assert scale[name] < 1e-6, (name, scale[name])
    print("checker gradient scales:", {k: f"{v:.1e}" for k, v in scale.items()})
    torch.testing.assert_close(loss.detach().cpu(), loss_o.detach(), rtol=1e-4, atol=0)
    assert scale["FE.sa1.mlp_convs.0.weight"] > 1e-5 and scale["FE.fp1.mlp_convs.0.weight"] > 1e-5   # not vacuous
    _check("paper extractor training step", errs, bound)
    opt = torch.optim.Adam([p for p in mine.parameters() if p.requires_grad], lr=1e-3)
    before = [mine_p[n].detach().clone() for n in ("FE.sa1.mlp_convs.0.weight", "FE.fp1.mlp_convs.0.weight")]
    opt.step()
    assert not torch.equal(before[0], mine_p["FE.sa1.mlp_convs.0.weight"].detach())
    assert not torch.equal(before[1], mine_p["FE.fp1.mlp_convs.0.weight"].detach())
    _, loss2 = run()
    assert torch.isfinite(loss2)


def test_train_extractor_guards(cuda):
    ref, src, tgt, R_gt, t_gt, starts = _pair()
    args = (src.to(cuda), tgt.to(cuda), R_gt.to(cuda), torch.zeros(1, 3))
    keys = ("vcp", "weights", "R", "t", "keypts", "score", "src_dfe", "tgt_dfe")
    plain = _mine(cuda)
    with torch.no_grad():
        off = plain(*args, starts=starts)
    # train_extractor=True under no_grad: today's inference bits, nothing carries a gradient
    mine = _mine(cuda, train_extractor=True)
    with torch.no_grad():
        quiet = mine(*args, starts=starts)
    for a, b in zip(quiet, off):
        for k in keys:
            assert torch.equal(a[k], b[k]) and not a[k].requires_grad, k
    # recorded: the same values
    rec = mine(*args, starts=starts)
    for a, b in zip(rec, off):
        assert a["vcp"].requires_grad and torch.equal(a["vcp"].detach(), b["vcp"])
        assert torch.equal(a["weights"].detach(), b["weights"]) and torch.equal(a["R"], b["R"])
    # train_heads alone with a trainable extractor parameter still raises
    heads = _mine(cuda, train_heads=True)
    with pytest.raises(NotImplementedError, match=r"extractor must be frozen \(model.FE.requires_grad_\(False\)\)"):
        heads(*args, starts=starts)
    # a frozen extractor under train_extractor=True is head training, bit for bit
    heads.FE.requires_grad_(False)
    mine.FE.requires_grad_(False)
    top = [st["topk"] for st in off]
    for m in (heads, mine):
        m.zero_grad()
        _loss(m, m(*args, starts=starts, keypoint_idx=top), R_gt, t_gt, cuda).backward()
    for (name, a), (_, b) in zip(heads.stages.named_parameters(), mine.stages.named_parameters()):
        assert a.grad is not None and torch.equal(a.grad, b.grad), name
    assert all(p.grad is None for p in mine.FE.parameters())
    # parameters with requires_grad=False get no gradient
    mine.FE.requires_grad_(True)
    mine.FE.fp2.requires_grad_(False)
    mine.FE.sa1.mlp_bns[0].bias.requires_grad_(False)
    mine.zero_grad()
    _loss(mine, mine(*args, starts=starts, keypoint_idx=top), R_gt, t_gt, cuda).backward()
    for name, p in mine.FE.named_parameters():
        assert (p.grad is None) == (not p.requires_grad), name
    with pytest.raises(NotImplementedError, match="training mode"):
        mine.train()(*args, starts=starts)
