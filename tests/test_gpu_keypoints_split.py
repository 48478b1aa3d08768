"""The split key-point stage (dvcp_src_keypoints_ws, csrc/keypoints_split.hip; 257 <= K <= 1024 by
default, any K <= 1024 with method="split") against the one-workgroup kernel and the CPU oracle."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]


def _close(got, want, tol, what, floor=1e-30):
    """max |got - want| <= tol * max |want| (tests/test_gpu_train.py's measure)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    scale = max(float(want.abs().max()), floor)
    err = float((got - want).abs().max())
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"
    return err / scale


def _rotations(B, seed):
    """B proper rotations (fp64) that are not the identity."""
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(B, 3, 3, dtype=torch.float64, generator=g))
    return q * torch.sign(torch.linalg.det(q)).view(B, 1, 1)


def _run(cuda, xyz, feat, top, kstart, R, dtype, method, ns=32):
    from dvcp import ops
    out = ops.src_keypoints(xyz.to(dtype).transpose(1, 2).contiguous().to(cuda), feat.to(cuda), top.to(cuda),
                            kstart.to(cuda), R.to(cuda), radius=1.0, nsample=ns, method=method)
    return [o.cpu() for o in out]


def _oracle(xyz, feat, top, kstart, R, ns=32):
    """index_points -> sample_and_group under fps_starts -> Get_Cat_Feat_Src, and deepVCP.py:86-91."""
    import oracle as O
    K = top.shape[1]
    kp = O.index_points(xyz, top)
    with O.fps_starts([kstart]):
        _, g_local, picked = O.sample_and_group(npoint=K, radius=1, nsample=ns, xyz=kp, points=None, returnidx=True)
    cat = O.Get_Cat_Feat_Src()(kp, g_local, O.index_points(feat, picked))
    Rr = R if R.shape[0] == xyz.shape[0] else R.repeat(xyz.shape[0], 1, 1)
    moved = torch.matmul(Rr, kp.permute(0, 2, 1).double()).permute(0, 2, 1)
    return kp, cat, moved


def _check_vs_oracle(got, want, dtype):
    kp, cat, moved = got
    kp_o, cat_o, moved_o = want
    assert kp.dtype == dtype and torch.equal(kp, kp_o)
    cat_o = cat_o.float()
    # the coordinate columns pin the FPS order and every ball list bit for bit
    assert torch.equal(cat[..., :3], cat_o[..., :3]), "FPS order or ball lists differ from the oracle"
    torch.testing.assert_close(cat[..., 3:], cat_o[..., 3:], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(moved, moved_o, rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------
# 1. split == lds, bit for bit

@functools.lru_cache(maxsize=None)
def _float_case(K, ns, B=3, seed=11, span=2.0):
    g = torch.Generator().manual_seed(seed + K)
    S = K + 40
    xyz = (torch.rand(B, S, 3, generator=g) * 2 - 1) * span
    feat = torch.randn(B, S, 32, generator=g)
    top = torch.stack([torch.randperm(S, generator=g)[:K] for _ in range(B)])
    kstart = torch.randint(0, K, (B,), generator=g)
    return xyz, feat, top, kstart


# [-2, 2]^3 gives short balls at these K (at most 30 hits at K = 256); the two [-1, 1]^3 cases add
# full ones (the scan's early exit)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("K,ns,span", [(32, 32, 2.0), (33, 32, 2.0), (64, 32, 2.0), (255, 32, 2.0), (256, 32, 2.0),
                                       (16, 16, 2.0), (255, 32, 1.0), (256, 32, 1.0)])
def test_split_equals_lds(cuda, K, ns, span, dtype):
    xyz, feat, top, kstart = _float_case(K, ns, span=span)
    kp = torch.gather(xyz, 1, top[..., None].expand(-1, -1, 3)).double()
    hits = (((kp[:, :, None, :] - kp[:, None, :, :]) ** 2).sum(-1) <= 1).sum(-1)
    assert int(hits.min()) < ns if span == 2.0 else int(hits.max()) > ns
    B = xyz.shape[0]
    for R in (_rotations(B, 5), _rotations(1, 6)):
        a = _run(cuda, xyz, feat, top, kstart, R, dtype, "lds", ns)
        b = _run(cuda, xyz, feat, top, kstart, R, dtype, "split", ns)
        for name, x, y in zip(("keypts", "src_cat", "moved"), a, b):
            assert x.shape == y.shape and x.dtype == y.dtype
            assert torch.equal(x, y), f"{name} differs between the LDS kernel and the split path"


# ------------------------------------------------------------------------------------------------
# 2. dyadic clouds against the oracle: every distance and the r^2 boundary exact in fp32

DYADIC = [(257, 1), (320, 4), (1000, 4), (1024, 16), (1024, 1)]


@functools.lru_cache(maxsize=None)
def _dyadic_case(K, scale, B=2, seed=3):
    g = torch.Generator().manual_seed(seed + 7 * K + scale)
    S = K + 40
    xyz = torch.randint(-64 * scale, 64 * scale, (B, S, 3), generator=g).double() / 64
    feat = torch.randn(B, S, 32, generator=g)
    top = torch.stack([torch.randperm(S, generator=g)[:K] for _ in range(B)])
    kstart = torch.randint(0, K, (B,), generator=g)
    for b in range(B):   # a duplicate key point per pair (FPS and ball-query ties)
        xyz[b, top[b, 17]] = xyz[b, top[b, 5]]
    R = _rotations(B, 9)
    kp = torch.gather(xyz, 1, top[..., None].expand(-1, -1, 3))
    d2 = ((kp[:, :, None, :] - kp[:, None, :, :]) ** 2).sum(-1)    # exact in fp64
    hits = (d2 <= 1).sum(-1)
    on_radius = int((d2 == 1).sum())
    dup = int((d2 == 0).sum()) - B * K
    want = {dt: _oracle(xyz.to(dt), feat, top, kstart, R) for dt in DTYPES}
    return (xyz, feat, top, kstart, R), want, (int(hits.min()), int(hits.max()), on_radius, dup)


def test_dyadic_cases_cover_the_regimes():
    """CPU: one case with every ball shorter than nsample, one with none shorter, one with a pair
    exactly on the radius, duplicates in all."""
    stats = {c: _dyadic_case(*c)[2] for c in DYADIC}
    print("hits per centre (min, max), pairs at d2 == 1, duplicate pairs:", stats)
    assert any(hi < 32 for _, hi, _, _ in stats.values())
    assert any(lo >= 32 for lo, _, _, _ in stats.values())
    assert any(lo < 32 <= hi for lo, hi, _, _ in stats.values())
    assert any(on > 0 for _, _, on, _ in stats.values())
    assert all(dup > 0 for _, _, _, dup in stats.values())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("K,scale", DYADIC)
def test_split_vs_oracle_dyadic(cuda, K, scale, dtype):
    from dvcp import ops
    assert ops.src_keypoints_method(K) == "split"
    (xyz, feat, top, kstart, R), want, _ = _dyadic_case(K, scale)
    got = _run(cuda, xyz, feat, top, kstart, R, dtype, None)
    _check_vs_oracle(got, want[dtype], dtype)


# ------------------------------------------------------------------------------------------------
# 3. random floats against the oracle

@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_split_vs_oracle_random_floats(cuda, dtype):
    K, B, S = 700, 2, 740
    g = torch.Generator().manual_seed(2)
    xyz = torch.rand(B, S, 3, generator=g) * 6 - 3
    feat = torch.randn(B, S, 32, generator=g)
    top = torch.stack([torch.randperm(S, generator=g)[:K] for _ in range(B)])
    kstart = torch.randint(0, K, (B,), generator=g)
    kp = torch.gather(xyz, 1, top[..., None].expand(-1, -1, 3)).double()
    d2 = ((kp[:, :, None, :] - kp[:, None, :, :]) ** 2).sum(-1)
    assert float((d2 - 1).abs().min()) > 1e-5, "a pair of key points lies within 1e-5 of r^2: pick another seed"
    R = _rotations(B, 2)
    got = _run(cuda, xyz, feat, top, kstart, R, dtype, None)
    _check_vs_oracle(got, _oracle(xyz.to(dtype), feat, top, kstart, R), dtype)


# ------------------------------------------------------------------------------------------------
# 4. gradient of the source features

@pytest.mark.parametrize("K", [320, 1024])
def test_feature_grad_vs_oracle(cuda, K):
    import oracle as O
    from dvcp import autograd
    g = torch.Generator().manual_seed(10 + K)
    B, S, ns = 2, K + 40, 32
    xyz = torch.rand(B, S, 3, generator=g) * 4 - 2
    feat = torch.rand(B, S, 32, generator=g)
    top = torch.stack([torch.randperm(S, generator=g)[:K] for _ in range(B)])
    kstart = torch.randint(0, K, (B,), generator=g)
    G = torch.randn(B, K, ns, 35, generator=g)
    fo = feat.clone().requires_grad_()
    kp = O.index_points(xyz, top)
    with O.fps_starts([kstart]):
        _, g_local, picked = O.sample_and_group(npoint=K, radius=1, nsample=ns, xyz=kp, points=None, returnidx=True)
    cat_o = O.Get_Cat_Feat_Src()(kp, g_local, O.index_points(fo, picked))
    (cat_o * G).sum().backward()
    fg = feat.to(cuda).requires_grad_()
    R = torch.eye(3, dtype=torch.float64, device=cuda)[None]
    _, cat, _ = autograd.src_keypoints(xyz.to(cuda).transpose(1, 2).contiguous(), fg, top.to(cuda), kstart.to(cuda), R)
    torch.testing.assert_close(cat.cpu(), cat_o.float(), rtol=1e-5, atol=1e-6)
    (cat * G.to(cuda)).sum().backward()
    _close(fg.grad, fo.grad, 1e-5, "d source features")
    assert not bool(fg.grad[:, K:].any()), "FE rows >= K received a gradient (Q4: key-point-local indices)"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("K", [48, 256])
def test_backward_ws_vs_lds_backward(cuda, K, dtype):
    from dvcp import ops
    xyz, feat, top, kstart = _float_case(K, 32, B=2, seed=21)
    B, S = xyz.shape[0], xyz.shape[1]
    G = torch.randn(B, K, 32, 35, generator=torch.Generator().manual_seed(K)).to(cuda)
    x = xyz.to(dtype).transpose(1, 2).contiguous().to(cuda)
    R = torch.eye(3, dtype=torch.float64, device=cuda)[None]
    want = ops.src_keypoints_backward(x, top.to(cuda), kstart.to(cuda), G)
    *_, ws = ops.src_keypoints(x, feat.to(cuda), top.to(cuda), kstart.to(cuda), R, method="split",
                               return_workspace=True)
    got = ops.src_keypoints_backward_ws(ws, S, K, G, dtype=dtype)
    assert got.shape == want.shape == (B, S, 32)
    _close(got, want, 1e-6, "d source features, workspace backward against the LDS backward")
    assert not bool(got[:, K:].any())


# ------------------------------------------------------------------------------------------------
# 5. end to end, inference

@pytest.mark.parametrize("K", [320, 1024])
def test_e2e_inference_vs_oracle(cuda, K):
    """test_e2e_large_grid_vs_oracle's recipe at K > 256 (r = 1.0, s = 0.4: G = 6): the oracle's top-k
    fed in, key points and candidates exact, the kNN of the first 4096 queries exact, the rest within
    the usual bars.  A K cap in a later stage would surface here."""
    import dvcp
    import oracle as O
    from dvcp.synthetic import condition_weights, make_pairs, randomize_bn
    from tests_helpers import topk_parity
    B, N = 1, 2048
    src, tgt, R, t = make_pairs(B, N, seed=71)
    torch.manual_seed(0)
    ref = O.DeepVCP(use_normal=False, K=K, r=1.0, s=0.4, fe_npoint=1024).eval()
    randomize_bn(ref)
    with torch.no_grad():
        _, calib = ref.FE1(src)
    condition_weights(ref, feats=calib)
    mine = dvcp.DeepVCP(use_normal=False, K=K, r=1.0, s=0.4, fe_npoint=1024).eval()
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
    C = 6 ** 3
    assert tr["cand"].shape == (B, K, C, 3)
    assert torch.equal(kp.cpu(), kp_o)
    assert torch.equal(tr["cand"].cpu(), d["candidates"])
    torch.testing.assert_close(tr["src_cat"].cpu(), d["src_cat"].float(), rtol=0, atol=1e-4)
    nq = 4096
    assert torch.equal(tr["knn_idx"][:, :nq].cpu().long(), d["knn_idx"][:, :nq]), "kNN indices differ from the oracle"
    assert torch.equal(tr["knn_dist"][:, :nq].cpu(), d["knn_dist"][:, :nq]), "kNN distances differ from the oracle"
    torch.testing.assert_close(tr["tgt_dfe"].cpu().reshape(d["tgt_dfe"].shape), d["tgt_dfe"], rtol=1e-4, atol=1e-5)
    print(f"e2e K={K}: max|vcp err| {float((vcp.cpu() - vcp_o).abs().max()):.2e}, "
          f"max|dR| {float((Rp.cpu() - R_o).abs().max()):.2e}, max|dt| {float((tp.cpu() - t_o).abs().max()):.2e}")
    torch.testing.assert_close(vcp.cpu(), vcp_o, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(Rp.cpu(), R_o, rtol=0, atol=1e-4)
    torch.testing.assert_close(tp.cpu(), t_o, rtol=0, atol=1e-4)
    if K == 320:   # the model's own top-k (dvcp_topk at K > 256) feeding the split stage
        tr2 = {}
        with torch.no_grad():
            kp2, _ = mine(src.to(cuda), tgt.to(cuda), R.to(cuda), torch.zeros(1, 3), starts=starts, trace=tr2)
        exact, n_amb = topk_parity(tr2["topk"], tr2["score"], d["topk_idx"], d["wl_score"][..., 0], K)
        print(f"e2e K={K}: GPU top-k == oracle top-k: {exact} ({n_amb} near-tie rank boundaries)")
        assert kp2.shape == (B, K, 3)
        if exact:
            assert torch.equal(kp2.cpu(), kp_o)


# ------------------------------------------------------------------------------------------------
# 6. end to end, training

def test_e2e_training_step_vs_oracle(cuda):
    """test_head_train_step_vs_oracle's recipe at K = 320, then the same model with FE1 trainable
    (frozen BN): the source features' gradient passes through dvcp_src_keypoints_backward_ws."""
    import dvcp
    import oracle as O
    from dvcp.synthetic import condition_weights, make_pairs, randomize_bn
    K = 320
    src, tgt, R_gt, t_gt = make_pairs(1, 1024, seed=91)
    torch.manual_seed(0)
    ref = O.DeepVCP(use_normal=False, K=K, r=1.0, s=0.4, fe_npoint=512)
    randomize_bn(ref)
    ref.FE1.eval()
    with torch.no_grad():
        _, calib = ref.FE1(src)
    condition_weights(ref, feats=calib)
    ref.FE1.requires_grad_(False)
    mine = dvcp.DeepVCP(use_normal=False, K=K, r=1.0, s=0.4, fe_npoint=512)
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
    torch.testing.assert_close(loss.detach().cpu(), loss_o.detach(), rtol=1e-4, atol=1e-6)
    errs = {}
    for mod in ("DFE.fc1", "DFE.fc2", "DFE.fc3", "cpg.conv1", "cpg.conv2", "cpg.conv3"):
        a, b = mod.split(".")
        for p in ("weight", "bias"):
            got = getattr(getattr(getattr(mine, a), b), p).grad
            want = getattr(getattr(getattr(ref, a), b), p).grad
            errs[f"{mod}.{p}"] = _close(got, want, 1e-3, f"{mod}.{p}",
                                        floor=1e-3 if (mod, p) == ("cpg.conv3", "bias") else 1e-30)
    print("relative gradient errors:", {k: f"{v:.1e}" for k, v in errs.items()})
    assert all(p.grad is None for p in mine.FE1.parameters())

    mine.zero_grad(set_to_none=True)
    mine.FE1.requires_grad_(True)
    mine.FE1.eval()
    torch.manual_seed(1)
    kp, vcp = mine(src.to(cuda), tgt.to(cuda), R_gt.to(cuda), torch.zeros(1, 3), keypoint_idx=top)
    dvcp.deepVCP_loss(kp, vcp, R_gt.to(cuda), t_gt.to(cuda), 0.5)[0].backward()
    for name, p in mine.FE1.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), name


# ------------------------------------------------------------------------------------------------
# 7. edges

def test_k_above_the_limit_raises_before_any_launch(cuda, monkeypatch):
    import dvcp
    from dvcp import _lib, ops
    log = []
    monkeypatch.setattr(_lib, "EVENT_LOG", log)
    S = 1100
    with pytest.raises(ValueError, match="1024"):
        ops.src_keypoints(torch.zeros(1, 3, S, device=cuda), torch.zeros(1, S, 32, device=cuda),
                          torch.zeros(1, 1025, dtype=torch.long, device=cuda), torch.zeros(1, dtype=torch.long),
                          torch.eye(3, dtype=torch.float64, device=cuda)[None])
    m = dvcp.DeepVCP(use_normal=False, K=1025, fe_npoint=1100).to(cuda).eval()
    x = torch.rand(1, 3, 2048, device=cuda)
    with torch.no_grad(), pytest.raises(ValueError, match="1024"):
        m(x, x, torch.eye(3, dtype=torch.float64, device=cuda)[None], torch.zeros(1, 3))
    assert log == [], "an entry point was called before the guard"


def test_unknown_method(cuda):
    from dvcp import ops
    xyz, feat, top, kstart = _float_case(64, 32)
    with pytest.raises(ValueError, match="nope"):
        _run(cuda, xyz, feat, top, kstart, _rotations(1, 1), torch.float32, "nope")


def test_k_equals_s_and_empty_batch(cuda):
    from dvcp import ops
    K = S = 1024
    g = torch.Generator().manual_seed(4)
    xyz = torch.randint(-256, 256, (1, S, 3), generator=g).double() / 64
    feat = torch.randn(1, S, 32, generator=g)
    top = torch.randperm(S, generator=g)[None]
    kstart = torch.tensor([K - 1])
    R = _rotations(1, 3)
    got = _run(cuda, xyz, feat, top, kstart, R, torch.float32, None)
    _check_vs_oracle(got, _oracle(xyz.float(), feat, top, kstart, R), torch.float32)
    kp, cat, moved, ws = ops.src_keypoints(torch.zeros(0, 3, S, device=cuda), torch.zeros(0, S, 32, device=cuda),
                                           torch.zeros(0, 512, dtype=torch.long, device=cuda),
                                           torch.zeros(0, dtype=torch.long, device=cuda), R.to(cuda),
                                           return_workspace=True)
    assert kp.shape == (0, 512, 3) and cat.shape == (0, 512, 32, 35) and moved.shape == (0, 512, 3)
    gF = ops.src_keypoints_backward_ws(ws, S, 512, torch.zeros(0, 512, 32, 35, device=cuda))
    assert gF.shape == (0, S, 32)


def test_two_streams_equal_serial_calls(cuda):
    """Two calls at K = 512 issued on two streams equal the same calls one after the other: each
    call has its own workspace."""
    from dvcp import ops
    K, B = 512, 2
    cases = []
    for seed in (31, 32):
        g = torch.Generator().manual_seed(seed)
        S = K + 40
        xyz = (torch.rand(B, 3, S, generator=g) * 6 - 3).to(cuda)
        feat = torch.randn(B, S, 32, generator=g).to(cuda)
        top = torch.stack([torch.randperm(S, generator=g)[:K] for _ in range(B)]).to(cuda)
        kstart = torch.randint(0, K, (B,), generator=g).to(cuda)
        cases.append((xyz, feat, top, kstart, _rotations(B, seed).to(cuda)))
    serial = [ops.src_keypoints(*c) for c in cases]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=cuda) for _ in cases]
    both = []
    for s, c in zip(streams, cases):
        with torch.cuda.stream(s):
            both.append(ops.src_keypoints(*c))
    torch.cuda.synchronize()
    for a, b in zip(serial, both):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
