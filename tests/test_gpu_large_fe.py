"""The model with more than 16384 feature points (DeepVCP(fe_npoint=16400) on 20000-point clouds):
the first forward whose top-k row, kNN reference set, target feature table and set-abstraction
centre lists all exceed 16384 entries.  One forward (module fixture), then each stage that meets the
larger tables against an independent statement of it: numpy's lexsort, the brute-force kNN, the
oracle's target stage, and the oracle's set-abstraction pieces on a sample of centres.  The oracle's
full feature extractor at this size takes minutes on the CPU and is not run; the weights are
calibrated on the GPU model's own features."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, N, K, R_, S_, NPOINT = 1, 20000, 32, 1.0, 0.4, 16400
G = 6                                                          # int(2 r / s + 1); C = 216 candidates


@pytest.fixture(scope="module")
def big(cuda):
    import dvcp
    from dvcp.synthetic import condition_weights, make_pairs, randomize_bn
    src, tgt, R_gt, t_gt = make_pairs(B, N, seed=1620)
    torch.manual_seed(0)
    mine = dvcp.DeepVCP(use_normal=False, K=K, r=R_, s=S_, fe_npoint=NPOINT).eval()
    randomize_bn(mine)
    mine.to(cuda)
    starts = mine.draw_starts(B, N, N)
    with torch.no_grad():
        calib = mine.extract_features(src.to(cuda), tgt.to(cuda), starts)["src_feat"]
    condition_weights(mine, feats=calib)                       # separated key-point scores
    tr = {}
    with torch.no_grad():
        kp, vcp = mine(src.to(cuda), tgt.to(cuda), R_gt.to(cuda), torch.zeros(1, 3), starts=starts, trace=tr)
    torch.cuda.synchronize()
    return dict(mine=mine, src=src, tgt=tgt, trace=tr, kp=kp, vcp=vcp)


def test_large_fe_forward_properties(cuda, big):
    tr, kp, vcp = big["trace"], big["kp"], big["vcp"]
    assert tr["src_xyz"].shape == (B, 3, NPOINT) and tr["tgt_xyz"].shape == (B, 3, NPOINT)
    assert tr["tgt_feat"].shape == (B, NPOINT, 32) and tr["score"].shape == (B, NPOINT)
    assert kp.shape == (B, K, 3) and vcp.shape == (B, K, 3)
    pts = big["src"][0].t().to(cuda)                           # (N, 3)
    member = (kp[0][:, None, :] == pts[None, :, :]).all(-1).any(-1)
    assert bool(member.all())                                  # every key point is a source point
    fe_pts = tr["src_xyz"][0].t()
    assert bool((fe_pts[::41, None, :] == pts[None, :, :]).all(-1).any(-1).all())   # (a sample of 400)
    assert len(torch.unique(fe_pts, dim=0)) == NPOINT          # FPS picked 16400 distinct points
    assert torch.isfinite(vcp).all()
    assert tr["cand"].shape == (B, K, G ** 3, 3)
    lo, hi = tr["cand"].amin(dim=2), tr["cand"].amax(dim=2)
    assert bool(((vcp >= lo - 1e-5) & (vcp <= hi + 1e-5)).all())   # a convex combination of candidates


def test_large_fe_topk_is_the_lexsort(cuda, big):
    tr = big["trace"]
    got = tr["topk"].cpu().numpy()
    for b in range(B):
        v = tr["score"][b].cpu().numpy()
        want = np.lexsort((np.arange(NPOINT), -v))[:K]
        assert np.array_equal(got[b], want)
    assert int(tr["topk"].max()) < NPOINT


def test_large_fe_knn_equals_brute(cuda, big):
    from dvcp import ops
    tr = big["trace"]
    qry = tr["cand"].view(B, -1, 3)
    d, i, _ = ops.knn(tr["tgt_xyz"], qry, 32, ref_pdim=2, qry_pdim=1, want_idx64=False, method="brute")
    assert torch.equal(tr["knn_idx"], i) and torch.equal(tr["knn_dist"], d)
    assert int(i.max()) >= 16384                               # the lists reach past the old limit


def test_large_fe_target_stage_vs_oracle(cuda, big):
    """kNN bit-equal and the fused target gather + DFE (dvcp_dfe_tgt gathering from a table of more
    than 16384 rows) within 1e-5 of the oracle, for the first 4 key points."""
    import oracle as O
    tr, mine = big["trace"], big["mine"]
    C, n = G ** 3, 4
    dfe_o = O.feat_embedding_layer()
    dfe_o.load_state_dict({k: v.cpu() for k, v in mine.DFE.state_dict().items()})
    tx, tf = tr["tgt_xyz"].transpose(1, 2).cpu(), tr["tgt_feat"].cpu()
    with torch.no_grad(), O.tracing() as trace:
        cat_o = O.Get_Cat_Feat_Tgt()(tr["cand"][:, :n].cpu(), tr["keypts"][:, :n].cpu(), tx, tf)
        want = dfe_o(cat_o, src=False)
    d = dict(trace)
    assert torch.equal(tr["knn_idx"][:, :n * C].cpu().long(), d["knn_idx"])
    assert torch.equal(tr["knn_dist"][:, :n * C].cpu(), d["knn_dist"])
    assert int(d["knn_idx"].max()) >= 16384
    torch.testing.assert_close(tr["tgt_dfe"][:, :n].cpu(), want, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("layer", ["sa1", "sa2", "sa3"])
def test_large_fe_set_abstraction_over_16384_centres(cuda, big, layer):
    """One set-abstraction layer standalone on 16400 points, every one a centre (npoint = 16400):
    256 centres spread over the FPS order against the oracle's pieces (ball query, grouping, the
    layer's convs and eval-mode BatchNorms, max) with the same weights.  Centres with a point within
    4 ulp of r^2 (where the oracle's BLAS-rounded d2 and the kernel's may disagree on membership,
    tests_helpers.ball_rows_mismatch_ok) are left out: at most 8."""
    import oracle as O
    import torch.nn.functional as F
    sa = getattr(big["mine"].FE1, layer)
    D = sa.chans[0] - 3
    g = torch.Generator().manual_seed(1621)
    xyz = big["src"][:, :, :NPOINT].contiguous()               # (1, 3, 16400), uniform in the cube
    points = torch.randn(B, D, NPOINT, generator=g) if D else None
    start = torch.tensor([777])
    with torch.no_grad():
        new_xyz, out = sa(xyz.to(cuda), points.to(cuda) if D else None, start=start)
    assert new_xyz.shape == (B, 3, NPOINT) and out.shape == (B, sa.chans[-1], NPOINT)
    pick = torch.linspace(0, NPOINT - 1, 256).long()
    ctr = new_xyz[:, :, pick].transpose(1, 2).cpu()            # (1, 256, 3)
    pts = xyz.transpose(1, 2)                                  # (1, 16400, 3)
    assert bool((ctr[0][:, None, :] == pts[0][None, :, :]).all(-1).any(-1).all())
    r2 = float(torch.tensor(sa.radius ** 2, dtype=torch.float32))
    near = ((O.square_distance(ctr, pts) - r2).abs() <= 4 * torch.finfo(torch.float32).eps * r2).any(-1)[0]
    assert int(near.sum()) <= 8, int(near.sum())
    ref = O.PointNetSetAbstraction(sa.npoint, sa.radius, sa.nsample, sa.chans[0], sa.chans[1:]).eval()
    ref.load_state_dict({k: v.cpu() for k, v in sa.state_dict().items()})
    with torch.no_grad():
        gidx = O.query_ball_point(sa.radius, sa.nsample, pts, ctr)
        grouped = O.index_points(pts, gidx) - ctr.view(B, 256, 1, 3)
        if D:
            grouped = torch.cat([grouped, O.index_points(points.transpose(1, 2), gidx)], dim=-1)
        x = grouped.permute(0, 3, 2, 1)
        for conv, bn in zip(ref.mlp_convs, ref.mlp_bns):
            x = F.relu(bn(conv(x.float())))
        want = torch.max(x, 2)[0]                              # (1, C', 256)
    keep = ~near
    torch.testing.assert_close(out[:, :, pick].cpu()[:, :, keep], want[:, :, keep], rtol=1e-4, atol=1e-5)
