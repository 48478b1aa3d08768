"""Pose solve (csrc/rigid.hip) at the inputs where an SVD-based solve goes wrong: rank-deficient
sets (n = 1..3, coplanar, collinear, identical points, at most three non-zero weights), repeated
and near-repeated singular values, inlier-rank ties, the n = 1024 LDS boundary and large offsets.

The reference is numpy fp64 in this file (centroids, H, np.linalg.svd; np.longdouble accumulation
for the offset cases).  LAPACK's null-space vectors are arbitrary, so for a rank-deficient H there
is no element-wise parity; ``_check_pose`` asserts what defines R = V U^T instead: R, t finite,
|R^T R - I| <= 1e-12, tr(R H) >= sigma_1 + sigma_2 + d sigma_3 - 1e-12 sigma_1 (R maximises
tr(R H); d = -1 only for the reflection-fixed solve of a mirrored set), t = cy - R cx, and
R = V diag(1, 1, d) U^T where sigma_3 / sigma_1 > 1e-6 makes R unique.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EYE = np.eye(3)
TINY = np.finfo(np.float64).tiny

# R against the longdouble-accumulated reference at coordinate offsets 1e3 and 1e5: 8 x the distance
# of a numpy fp64 two-pass solve (the kernel's formula: centroids, then H of the centred points)
# from that reference on the sets of test_rigid_offsets_and_scales, floor 1e-12.
#   measured max |R_fp64 - R_longdouble| (two_pass_fp64_vs_longdouble, exact and noisy pairs):
#   offset 1e3: 8.9e-16, offset 1e5: 1.6e-15 (offset 0: 6.7e-16) -- centring x - cx is exact for
#   coordinates this close to the centroid, and the centroid's own error cancels in H to first order.
# Offset 0 and the scaled sets keep the project's 1e-9.
OFFSET_TOL = {0.0: 1e-9, 1e3: max(8 * 8.9e-16, 1e-12), 1e5: max(8 * 1.6e-15, 1e-12)}


# ------------------------------------------------------------------------------------ helpers
def _rot(g, proper=True):
    q = np.linalg.qr(g.standard_normal((3, 3)))[0]
    q = q * np.sign(np.linalg.det(q))
    return q if proper else q @ np.diag([1.0, 1.0, -1.0])


def _small_rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return EYE + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _dyadic(g, shape, bits=5, span=4):
    """Random multiples of 2^-bits in [-span, span]: sums and centroids of a few of them are exact."""
    return g.integers(-span * 2 ** bits, span * 2 ** bits + 1, shape) / 2.0 ** bits


def _close(got, want, tol, what):
    """max |got - want| <= tol * max |want| (test_gpu_train._close)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    scale = max(float(want.abs().max()), 1e-30)
    err = float((got - want).abs().max())
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ref(x, y, w=None, acc=np.float64):
    """x, y (3, n), w (n,) -> H, cx, cy (fp64, accumulated in ``acc``) and np.linalg.svd(H)."""
    xa, ya = np.asarray(x, acc), np.asarray(y, acc)
    wa = np.ones(xa.shape[1], acc) if w is None else np.asarray(w, acc)
    W = wa.sum()
    cx, cy = (xa * wa).sum(1) / W, (ya * wa).sum(1) / W
    H = ((xa - cx[:, None]) * wa) @ (ya - cy[:, None]).T
    H, cx, cy = np.asarray(H, np.float64), np.asarray(cx, np.float64), np.asarray(cy, np.float64)
    U, s, Vt = np.linalg.svd(H)
    return H, cx, cy, U, s, Vt


def _check_pose(name, R, t, x, y, w=None, fix=False, acc=np.float64, tol_R=1e-9):
    """The property checks of the module docstring on one pair; returns sigma."""
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3)
    H, cx, cy, U, s, Vt = _ref(x, y, w, acc)
    assert np.isfinite(R).all() and np.isfinite(t).all(), (name, R, t)
    orth = np.abs(R.T @ R - EYE).max()
    assert orth <= 1e-12, (name, "R^T R - I", orth)
    d = np.sign(np.linalg.det(Vt.T @ U.T)) if fix else 1.0
    bound = s[0] + s[1] + d * s[2]
    gap = bound - np.trace(R @ H)
    assert gap <= 1e-12 * max(s[0], TINY), (name, "tr(RH) below sum sigma by", gap, s)
    c = max(np.abs(cx).max(), np.abs(cy).max())
    terr = np.abs(t - (cy - R @ cx)).max()
    assert terr <= 1e-12 * (1 + c), (name, "t - (cy - R cx)", terr)
    if s[0] > 0 and s[2] / s[0] > 1e-6:
        err = np.abs(R - Vt.T @ np.diag([1.0, 1.0, d]) @ U.T).max()
        assert err <= tol_R, (name, "R - V U^T", err, tol_R)
    return s


def _check_exact_fit(name, R, t, x, y):
    """Exact rigid input under a proper rotation: the returned pose reproduces y (also for coplanar
    and collinear sets, where the returned proper rotation is optimal on the span of the points)."""
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)
    scale = max(np.abs(x - x.mean(1, keepdims=True)).max(), np.abs(y - y.mean(1, keepdims=True)).max())
    res = np.abs(R @ x + t - y).max()
    floor = 8 * np.finfo(np.float64).eps * np.abs(y).max()      # forming R x + t here, in fp64, rounds that much
    assert res <= 1e-9 * scale + floor, (name, "max |R x + t - y|", res, scale)


def _rigid_gpu(x, y, cuda):
    import dvcp
    R, t = dvcp.get_rigid_transform(_T(x, cuda), _T(y, cuda))
    return R.cpu().numpy(), t.cpu().numpy()


def _pair(g, x, noise, proper=True, R_true=None):
    R_true = _rot(g, proper) if R_true is None else R_true
    t_true = g.standard_normal((3, 1))
    y = R_true @ x + t_true
    if noise:
        y = y + noise * g.standard_normal(y.shape)
    return y


# ---- point sets (3, n) ----
def _coplanar(g, n):
    x = _dyadic(g, (3, n))
    x[2] = 0.0
    return x


def _collinear(g, n):
    k = g.integers(-16, 17, n).astype(np.float64)
    k[:2] = (-16, 16)
    return np.array([[1.0], [0.5], [-0.25]]) * k + np.array([[0.5], [-1.0], [2.0]])


def _identical(g, n):
    return np.repeat(_dyadic(g, (3, 1)), n, axis=1)


def _near_coplanar(g, n, thick):
    x = g.uniform(-1, 1, (3, n))
    x[2] *= thick
    return x


CUBE = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64).T
OCTA = np.concatenate([np.eye(3), -np.eye(3)], 1)
PRISM = CUBE * np.array([[1.0], [1.0], [2.0]])


def _tile(x, n):
    return np.tile(x, (1, n // x.shape[1]))


# ---------------------------------------------------------------- (a) get_rigid_transform
@pytest.mark.parametrize("noise", [0.0, 0.01], ids=["exact", "noisy"])
def test_rigid_sizes(cuda, noise):
    """n = 1, 2, 3 (rank 0, 1, 2 by construction), 4, the 256-thread strides, 1024 / 1025 and 4000."""
    g = np.random.default_rng(201)
    for n in (1, 2, 3, 4, 255, 256, 257, 513, 1024, 1025, 4000):
        x = g.standard_normal((3, 3, n))
        y = np.stack([_pair(g, x[b], noise) for b in range(3)])
        R, t = _rigid_gpu(x, y, cuda)
        for b in range(3):
            s = _check_pose((n, b), R[b], t[b], x[b], y[b])
            assert n > 3 or s[n - 1] <= 1e-14 * max(s[0], TINY), (n, s)   # the rank this n was built for
            if not noise:
                _check_exact_fit((n, b), R[b], t[b], x[b], y[b])


def _degenerate_rows(g, n, noise):
    """Rows 0 and 4 are generic full-rank neighbours."""
    kinds = [("generic0", g.standard_normal((3, n))), ("coplanar", _coplanar(g, n)), ("collinear", _collinear(g, n)),
             ("identical", _identical(g, n)), ("generic1", g.standard_normal((3, n))),
             ("near_coplanar_1e-3", _near_coplanar(g, n, 1e-3)), ("near_coplanar_1e-8", _near_coplanar(g, n, 1e-8)),
             ("near_coplanar_1e-13", _near_coplanar(g, n, 1e-13))]
    names = [k for k, _ in kinds]
    x = np.stack([v for _, v in kinds])
    y = np.stack([_pair(g, x[b], noise) for b in range(len(kinds))])
    return names, x, y


@pytest.mark.parametrize("noise", [0.0, 0.01], ids=["exact", "noisy"])
def test_rigid_degenerate_kinds(cuda, noise):
    """Coplanar, collinear, identical and near-coplanar sets in the rows of one call, between
    full-rank rows that must come out bit-identical to a call without the degenerate rows."""
    g = np.random.default_rng(202)
    names, x, y = _degenerate_rows(g, 24, noise)
    R, t = _rigid_gpu(x, y, cuda)
    for b, name in enumerate(names):
        s = _check_pose(name, R[b], t[b], x[b], y[b])
        if name == "coplanar":
            assert s[2] <= 1e-14 * s[0]
        if name == "collinear":
            assert s[1] <= 1e-14 * s[0]
        if name == "identical":
            assert s[0] == 0.0 and np.array_equal(R[b], EYE)
        if not noise:
            _check_exact_fit(name, R[b], t[b], x[b], y[b])
    Rn, tn = _rigid_gpu(x[[0, 4]], y[[0, 4]], cuda)
    assert np.array_equal(Rn, R[[0, 4]]) and np.array_equal(tn, t[[0, 4]])


@pytest.mark.parametrize("noise", [0.0, 0.01], ids=["exact", "noisy"])
def test_rigid_equal_singular_values(cuda, noise):
    """Cube and octahedron vertices under signed permutation matrices (three equal sigma; the
    octahedron's is a reflection, returned as-is, Q13) and a square prism (two equal sigma)."""
    g = np.random.default_rng(203)
    n = 24
    P_proper = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])
    P_mirror = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]) @ np.diag([1.0, -1.0, 1.0])
    assert np.linalg.det(P_proper) > 0 > np.linalg.det(P_mirror)
    rows = [("generic0", g.standard_normal((3, n)), None), ("cube", _tile(CUBE, n), P_proper),
            ("octahedron", _tile(OCTA, n), P_mirror), ("prism", _tile(PRISM, n), None),
            ("generic1", g.standard_normal((3, n)), None)]
    x = np.stack([v for _, v, _ in rows])
    y = np.stack([_pair(g, v, noise, R_true=P) for _, v, P in rows])
    R, t = _rigid_gpu(x, y, cuda)
    for b, (name, _, P) in enumerate(rows):
        s = _check_pose(name, R[b], t[b], x[b], y[b])
        if not noise:
            if name in ("cube", "octahedron"):
                assert s[0] - s[2] <= 1e-12 * s[0], (name, s)
                assert np.abs(R[b] - P).max() <= 1e-12, name
            if name == "prism":
                assert s[1] - s[2] <= 1e-12 * s[0] < s[0] - s[1], (name, s)
            if name != "octahedron":
                _check_exact_fit(name, R[b], t[b], x[b], y[b])
    Rn, tn = _rigid_gpu(x[[0, 4]], y[[0, 4]], cuda)
    assert np.array_equal(Rn, R[[0, 4]]) and np.array_equal(tn, t[[0, 4]])


def _offset_case(offset, scale, noise, seed=204, n=257):
    """Rows: three generic sets, a coplanar and a collinear one; the offset is added to both clouds
    of a pair formed at the origin, so an exact pair stays exact up to the rounding of the sum."""
    g = np.random.default_rng(seed)
    x0 = np.stack([g.standard_normal((3, n)), g.standard_normal((3, n)), g.uniform(-2, 2, (3, n)), _coplanar(g, n),
                   _collinear(g, n)])
    y0 = np.stack([_pair(g, x0[b], noise) for b in range(len(x0))])
    return (x0 * scale + offset), (y0 * scale + offset)


def two_pass_fp64_vs_longdouble(offset, noise):
    """max |R| distance of the fp64 two-pass solve (numpy) from the longdouble-accumulated one over
    the generic rows of ``_offset_case``: the measurement behind OFFSET_TOL."""
    x, y = _offset_case(offset, 1.0, noise)
    worst = 0.0
    for b in range(3):
        _, _, _, U, _, Vt = _ref(x[b], y[b])
        _, _, _, Ul, _, Vtl = _ref(x[b], y[b], acc=np.longdouble)
        worst = max(worst, np.abs(Vt.T @ U.T - Vtl.T @ Ul.T).max())
    return worst


@pytest.mark.parametrize("noise", [0.0, 0.01], ids=["exact", "noisy"])
@pytest.mark.parametrize("offset,scale", [(0.0, 1.0), (1e3, 1.0), (1e5, 1.0), (0.0, 1e-6), (0.0, 1e6)])
def test_rigid_offsets_and_scales(cuda, offset, scale, noise):
    """KITTI-scale coordinate offsets and coordinate scales 1e-6 / 1e6 against the
    longdouble-accumulated reference (R within OFFSET_TOL where it is unique)."""
    x, y = _offset_case(offset, scale, noise)
    R, t = _rigid_gpu(x, y, cuda)
    for b in range(len(x)):
        _check_pose((offset, scale, b), R[b], t[b], x[b], y[b], acc=np.longdouble, tol_R=OFFSET_TOL[offset])
        if not noise:
            _check_exact_fit((offset, scale, b), R[b], t[b], x[b], y[b])


# ----------------------------------------------------- (b) svd_optimization and deepVCP_loss
def _loss_case(B, n, seed):
    from dvcp.synthetic import make_pairs
    g = torch.Generator().manual_seed(seed)
    _, _, R_gt, t_gt = make_pairs(B, 8, seed=seed)
    x = torch.rand(B, n, 3, generator=g) * 2 - 1
    y = (torch.matmul(R_gt, x.double().transpose(1, 2)) + t_gt).transpose(1, 2)
    y = (y + 0.05 * torch.randn(B, n, 3, generator=g, dtype=torch.float64)).float()
    return x, y, R_gt, t_gt


@pytest.mark.parametrize("n", [5, 257, 300, 513, 1024])
def test_pose_loss_sizes_vs_oracle(cuda, n):
    """deepVCP_loss forward and backward past one and two 256-thread strides and at the LDS limit
    n = 1024, against the oracle at the bars of test_pose_loss_backward_vs_oracle."""
    import oracle as O
    import dvcp
    x, y, R_gt, t_gt = _loss_case(2, n, 300 + n)
    y_o = y.clone().requires_grad_()
    loss_o, R_o, t_o = O.deepVCP_loss(x, y_o, R_gt, t_gt, 0.5)
    loss_o.backward()
    y_g = y.to(cuda).requires_grad_()
    loss, R, t = dvcp.deepVCP_loss(x.to(cuda), y_g, R_gt.to(cuda), t_gt.to(cuda), 0.5)
    loss.backward()
    torch.testing.assert_close(loss.detach().cpu(), loss_o.detach(), rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(R.cpu(), R_o, rtol=0, atol=1e-10)
    torch.testing.assert_close(t.cpu(), t_o, rtol=0, atol=1e-10)
    _close(y_g.grad, y_o.grad, 1e-6, "d y_pred")
    with torch.no_grad():   # the plain forward entry (dvcp_deepvcp_loss) as well
        loss2, R2, _ = dvcp.deepVCP_loss(x.to(cuda), y.to(cuda), R_gt.to(cuda), t_gt.to(cuda), 0.5)
    torch.testing.assert_close(loss2, loss.detach(), rtol=1e-12, atol=0)
    assert torch.equal(R2, R)


@pytest.mark.parametrize("n,msg", [(1025, r"n=1025 unsupported \(1\.\.1024\)"), (1, r"int\(0\.8 n\) == 0")])
@pytest.mark.parametrize("grad", [False, True])
def test_pose_loss_rejects_sizes(cuda, n, msg, grad):
    """n = 1025 (past the LDS arrays) and n = 1 (no inlier) raise with the library's message before
    anything is launched: the device has no error afterwards."""
    import dvcp
    x, y, R_gt, t_gt = _loss_case(2, n, 7)
    y_g = y.to(cuda).requires_grad_(grad)
    with pytest.raises(RuntimeError, match=msg):
        dvcp.deepVCP_loss(x.to(cuda), y_g, R_gt.to(cuda), t_gt.to(cuda), 0.5)
    with pytest.raises(RuntimeError, match=msg):
        dvcp.svd_optimization(x.transpose(1, 2).double().to(cuda), y.transpose(1, 2).double().to(cuda), R_gt.to(cuda),
                              t_gt.to(cuda))
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [2, 3])
def test_pose_loss_tiny_n(cuda, n):
    """n = 2, 3: the second solve runs on int(0.8 n) = 1, 2 points (H of rank 0, 1).  R2, t2 pass
    the property checks on (x1, R1 x1 + t1); the loss and its gradient are finite."""
    import dvcp
    g = np.random.default_rng(210 + n)
    B = 4
    x = g.standard_normal((B, 3, n))
    R_true = np.stack([_rot(g) for _ in range(B)])
    t_true = g.standard_normal((B, 3, 1))
    y = R_true @ x + t_true + 0.05 * g.standard_normal((B, 3, n))
    dev = [_T(a, cuda) for a in (x, y, R_true, t_true)]
    R1, t1 = _rigid_gpu(x, y, cuda)
    R2, t2, x1, y2 = (a.cpu().numpy() for a in dvcp.svd_optimization(*dev))
    n_in = int(n * 0.8)
    assert x1.shape == (B, 3, n_in)
    for b in range(B):
        _check_pose(("R1", n, b), R1[b], t1[b], x[b], y[b])
        cols = [int(np.flatnonzero((x[b] == x1[b][:, k:k + 1]).all(0))[0]) for k in range(n_in)]
        assert len(set(cols)) == n_in
        y1 = (R1[b] @ x[b] + t1[b])[:, cols]
        _check_pose(("R2", n, b), R2[b], t2[b], x1[b], y1)
        assert np.abs(y2[b] - (R2[b] @ x1[b] + t2[b])).max() <= 1e-12
    yg = _T(y.transpose(0, 2, 1), cuda).requires_grad_()
    loss, R, t = dvcp.deepVCP_loss(_T(x.transpose(0, 2, 1), cuda), yg, dev[2], dev[3], 0.5)
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(R).all()) and bool(torch.isfinite(t).all())
    assert bool(torch.isfinite(yg.grad).all())
    assert np.abs(R.detach().cpu().numpy() - R2).max() <= 1e-14


# ---------------------------------------------------------------------------- (c) inlier ties
def _nn_f32(R1, t1, Rt, tt, x):
    """svd_opt_front's 1-NN distances: y1 and y_true cast to fp32, (dx^2 + dy^2) + dz^2 in fp32,
    the minimum over y1, then the correctly rounded fp32 sqrt."""
    rows = lambda R, t: np.stack([R[a, 0] * x[0] + R[a, 1] * x[1] + R[a, 2] * x[2] + t.reshape(3)[a] for a in range(3)])
    y1 = rows(R1, t1).astype(np.float32)       # element-wise (no BLAS): duplicated columns stay bit-identical
    yt = rows(Rt, tt).astype(np.float32)
    d = y1[:, None, :] - yt[:, :, None]                       # (3, query j, candidate i)
    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    assert d2.dtype == np.float32
    return np.sqrt(d2.min(1))


def test_svd_optimization_inlier_ties(cuda):
    """Duplicated columns in x and y_pred give exactly equal, non-zero 1-NN distances; a tied group
    straddles the int(0.8 n) cut (asserted here on the CPU).  The kernel ranks ties to the lower
    index and emits rank order: x1 must equal x[:, stable_argsort(d)[:n_in]] column by column (a
    tie rule that gave two columns one rank would leave a slot of the inlier list unwritten).
    Tied columns are identical, so the order inside a tied group is not observable; how many of
    its copies are kept, and every column's place, is."""
    import dvcp
    g = np.random.default_rng(220)
    B, m, n = 3, 13, 40                                       # 13 columns x 3 copies + 1 single
    n_in = int(n * 0.8)
    base = g.standard_normal((B, 3, m))
    x = np.concatenate([np.tile(base, (1, 1, 3)), g.standard_normal((B, 3, 1))], 2)
    R_true = np.stack([_rot(g) for _ in range(B)])
    t_true = g.standard_normal((B, 3, 1))
    yb = R_true @ x[:, :, :m] + t_true + 0.05 * g.standard_normal((B, 3, m))
    y = np.concatenate([np.tile(yb, (1, 1, 3)), 3.0 * g.standard_normal((B, 3, 1))], 2)   # the single: an outlier
    R1, t1 = _rigid_gpu(x, y, cuda)
    R2, t2, x1, y2 = (a.cpu().numpy() for a in dvcp.svd_optimization(*[_T(a, cuda) for a in (x, y, R_true, t_true)]))
    for b in range(B):
        d = _nn_f32(R1[b], t1[b], R_true[b], t_true[b], x[b])
        order = np.argsort(d, kind="stable")
        assert d[order[n_in - 1]] == d[order[n_in]] > 0, "the tied group must straddle the cut"
        vals = np.unique(d)
        assert (np.diff(vals) > 1e-4 * vals[1:]).all(), "distinct distances far apart: fp64 rounding of y1 cannot reorder"
        assert np.array_equal(x1[b], x[b][:, order[:n_in]]), b
        _check_pose(("ties", b), R2[b], t2[b], x1[b], (R1[b] @ x[b] + t1[b])[:, order[:n_in]])


def _residuals_elementwise(R, t, x, y):
    """|R x + t - y| per column without BLAS, so duplicated columns give bit-identical values."""
    e = [R[a, 0] * x[0] + R[a, 1] * x[1] + R[a, 2] * x[2] + t[a] - y[a] for a in range(3)]
    return np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])


@pytest.mark.parametrize("fix", [True, False])
def test_paper_pose_rejection_ties(cuda, fix):
    """paper_pose with inlier_ratio 0.8 on pairs with duplicated (x, y) columns of different
    weights: the fp64 residuals tie exactly, a tied group straddles the cut, and which copy is kept
    (the lower index) changes the second solve.  oracle/paper.py ranks with a stable argsort
    (lower index first), the kernel's rule; its kept set is checked here against a restatement
    whose residuals are formed element-wise (no BLAS, so the ties are exact), then R, t at 1e-9."""
    from oracle import paper as OP
    from dvcp import ops
    g = np.random.default_rng(221)
    B, m, n = 3, 13, 40
    n_in = int(0.8 * n)
    base = g.standard_normal((B, 3, m))
    x = np.concatenate([np.tile(base, (1, 1, 3)), g.standard_normal((B, 3, 1))], 2)
    R_true = np.stack([_rot(g) for _ in range(B)])
    yb = R_true @ base + g.standard_normal((B, 3, 1)) + 0.05 * g.standard_normal((B, 3, m))
    y = np.concatenate([np.tile(yb, (1, 1, 3)), 3.0 * g.standard_normal((B, 3, 1))], 2)
    w = g.random((B, n)) + 0.05
    R, t = ops.paper_pose(_T(x, cuda), _T(y, cuda), _T(w, cuda), reflection_fix=fix, inlier_ratio=0.8)
    R, t = R.cpu().numpy(), t.cpu().numpy()
    for b in range(B):
        R1, t1 = OP.weighted_rigid_transform(x[b], y[b], w[b], fix)
        res = _residuals_elementwise(R1, t1, x[b], y[b])
        order = np.argsort(res, kind="stable")
        assert res[order[n_in - 1]] == res[order[n_in]] > 0, "the tied group must straddle the cut"
        vals = np.unique(res)
        assert (np.diff(vals) > 1e-6 * vals[1:]).all()
        kept = np.sort(order[:n_in])
        hi = np.flatnonzero(res == res[order[n_in]])
        assert len(set(w[b][hi])) == len(hi) and not set(hi) <= set(kept)    # the choice matters
        R_o, t_o, keep_o = OP.paper_pose(x[b], y[b], w[b], 0.8, fix)
        assert np.array_equal(keep_o, kept), (b, keep_o, kept)
        assert np.abs(R[b] - R_o).max() <= 1e-9 and np.abs(t[b][:, 0] - t_o).max() <= 1e-9, b
        _check_pose(("paper ties", b), R[b], t[b], x[b][:, kept], y[b][:, kept], w[b][kept], fix=fix)


# ------------------------------------------------- (d) backward at repeated singular values
def _kabsch_np(x, y):
    H, cx, cy, U, _, Vt = _ref(x, y)
    R = Vt.T @ U.T
    return R, cy - R @ cx


def _loss_np(x, y, R_true, t_true, alpha, info=None):
    """deepVCP_loss.py:57-121 restated in numpy fp64 (fp32 1-NN distances as the kernel forms them).
    x, y (B, 3, n).  ``info`` collects per pair: sigma of both solves, the sorted distances, the
    residuals y2 - y_true1."""
    B, _, n = x.shape
    n_in = int(n * 0.8)
    diffs = []
    for b in range(B):
        R1, t1 = _kabsch_np(x[b], y[b])
        d = _nn_f32(R1, t1, R_true[b], t_true[b], x[b])
        sel = np.argsort(d, kind="stable")[:n_in]
        x1, y1 = x[b][:, sel], (R1 @ x[b] + t1[:, None])[:, sel]
        R2, t2 = _kabsch_np(x1, y1)
        diffs.append(R2 @ x1 + t2[:, None] - (R_true[b] @ x1 + t_true[b].reshape(3, 1)))
        if info is not None:
            info.append(dict(s1=_ref(x[b], y[b])[4], s2=_ref(x1, y1)[4], d=np.sort(d), diff=diffs[-1]))
    diff = np.stack(diffs)
    return alpha * np.abs(diff).mean() + (1 - alpha) * abs(diff.mean())


def _fd(f, a, h=1e-6):
    """Central finite differences of the scalar f in every entry of ``a``."""
    grad = np.zeros_like(a)
    for i in np.ndindex(a.shape):
        ap, am = a.copy(), a.copy()
        ap[i] += h
        am[i] -= h
        grad[i] = (f(ap) - f(am)) / (2 * h)
    return grad


def _null_noise(g, x, w, amp):
    """Noise N (3, n) with X W N^T = 0 and N W 1 = 0: it leaves H = sum w (x - cx)(y - cy)^T alone."""
    A = np.concatenate([x, np.ones((1, x.shape[1]))])                     # 4 x n
    G = amp * g.standard_normal(x.shape)
    return G - (G * w) @ A.T @ np.linalg.inv((A * w) @ A.T) @ A


def _symmetric_sets():
    """Sets whose first solve (all n points) has two equal sigma and whose second solve (the
    int(0.8 n) = n - 2 inliers, the symmetric body without the two far points on its axis) has
    three equal sigma (cube, octahedron), two equal (prism) or two within 1e-9 (box)."""
    far = lambda z: np.array([[0.0, 0.0], [0.0, 0.0], [z, -z]])
    box = CUBE * np.array([[1.0], [1.0 + 5e-10], [2.0]])
    return {"cube": np.concatenate([CUBE, far(3.0)], 1), "octahedron": np.concatenate([OCTA, far(2.5)], 1),
            "prism": np.concatenate([PRISM, far(4.0)], 1), "near_repeated": np.concatenate([box, far(4.0)], 1)}


@pytest.mark.parametrize("name", ["cube", "octahedron", "prism", "near_repeated"])
def test_pose_loss_backward_repeated_singular_values(cuda, name):
    """d loss / d y_pred where H has repeated (or 1e-9-close) singular values in both solves,
    against central finite differences (step 1e-6) of the numpy fp64 loss; torch's SVD backward
    divides by sigma_i^2 - sigma_j^2 there, so the oracle's autograd cannot be the reference.

    y_pred = R' x + t' + N: (R', t') is the true pose turned by 0.02 rad and shifted by 1 %, so no
    L1 residual is zero, and N is 1 % noise in the null space of [x; 1], so H = X X^T R'^T keeps
    its repeated values.  Asserted on the CPU: the relative sigma gaps; the cut between the kept
    and the rejected distances is wider than 1e-4 and every |residual| and |mean residual| exceeds
    1e-5, so within the step the selection is constant and the loss is smooth.  Bar: 1e-6 of the
    largest gradient entry (finite-difference error: truncation ~h^2 and rounding ~1e-16 / h,
    both below 1e-9 of it)."""
    import dvcp
    g = np.random.default_rng(230)
    x0 = _symmetric_sets()[name]
    n = x0.shape[1]
    B = 2
    Rs = [_rot(g) for _ in range(B)]                                       # the body in two orientations
    x = np.stack([Rb @ x0 + 0.0 for Rb in Rs])
    R_true = np.stack([_rot(g) for _ in range(B)])
    t_true = g.standard_normal((B, 3, 1))
    # the 0.02 rad turn is about a line across the body's axis, so the two far points move the most
    y = np.stack([R_true[b] @ _small_rot(Rs[b] @ np.array([1.0, 0.4, 0.1]), 0.02) @ x[b] + t_true[b]
                  + 0.003 * g.standard_normal((3, 1)) + _null_noise(g, x[b], np.ones(n), 0.01) for b in range(B)])
    info = []
    loss_np = _loss_np(x, y, R_true, t_true, 0.5, info)
    n_in = int(0.8 * n)
    for b, I in enumerate(info):
        s1, s2 = I["s1"], I["s2"]
        if name in ("cube", "octahedron"):
            assert s1[1] - s1[2] <= 1e-12 * s1[0] and s2[0] - s2[2] <= 1e-12 * s2[0], (s1, s2)
        elif name == "prism":
            assert s1[1] - s1[2] <= 1e-12 * s1[0] and s2[1] - s2[2] <= 1e-12 * s2[0], (s1, s2)
        else:
            for s in (s1, s2):
                assert 0.5e-9 < (s[1] - s[2]) / s[1] < 2e-9, s
        assert I["d"][n_in] - I["d"][n_in - 1] > 1e-4, I["d"]
        assert np.abs(I["diff"]).min() > 1e-5
    assert abs(np.stack([I["diff"] for I in info]).mean()) > 1e-5
    want = _fd(lambda yy: _loss_np(x, yy, R_true, t_true, 0.5), y)
    yg = _T(y.transpose(0, 2, 1), cuda).requires_grad_()
    loss, _, _ = dvcp.deepVCP_loss(_T(x.transpose(0, 2, 1), cuda), yg, _T(R_true, cuda), _T(t_true, cuda), 0.5)
    loss.backward()
    assert abs(float(loss.detach()) - loss_np) <= 1e-10 * abs(loss_np)
    _close(yg.grad, torch.from_numpy(want.transpose(0, 2, 1)), 1e-6, "d y_pred (finite differences)")


def _whitened(g, x0, w, D):
    """x with weighted centroid 0 and sum w x x^T = D^2 exactly (to rounding), for any weights."""
    xc = x0 - (x0 * w).sum(1, keepdims=True) / w.sum()
    lam, Q = np.linalg.eigh((xc * w) @ xc.T)
    return np.diag(D) @ (Q / np.sqrt(lam)) @ Q.T @ xc


@pytest.mark.parametrize("fix,mirror", [(True, False), (False, False), (False, True)])
@pytest.mark.parametrize("name", ["cube", "octahedron", "prism", "near_repeated"])
def test_paper_backward_repeated_singular_values(cuda, name, fix, mirror):
    """The paper backward (d loss / d y*, d loss / d w) at repeated singular values against central
    finite differences (step 1e-6) of oracle.paper.deepvcp_loss_paper, with weights in [0.05, 1.05)
    as test_gpu_paper._pose_case draws them.  Random weights break the symmetry of the cube,
    octahedron and prism, so each set is whitened under its weights (sum w x x^T = D^2, D = I for
    three equal sigma, diag(1, 1, 2) for two, diag(1, 1 + 5e-10, 2) for the 1e-9 gap), and the 1 %
    noise on y* is taken in the weighted null space of [x; 1] so H keeps those values; the pose
    behind y* is 0.02 rad and 1 % off the true one, so no L1 residual is zero (asserted > 1e-5).
    The mirrored case (no reflection fix) differentiates the improper polar factor.  The project's
    bar for this gradient is 1e-9 against autograd; finite differences carry ~1e-9 of error
    themselves (rounding 1e-16 / h against gradients of 1e-3), so the bar here is 1e-6."""
    from oracle import paper as OP
    import dvcp
    g = np.random.default_rng(240)
    x0 = _symmetric_sets()[name]
    n = x0.shape[1]
    B = 2
    D = {"cube": [1, 1, 1], "octahedron": [1, 1, 1], "prism": [1, 1, 2], "near_repeated": [1, 1 + 5e-10, 2]}[name]
    w = g.random((B, n)) + 0.05
    x = np.stack([_rot(g) @ _whitened(g, x0, w[b], np.array(D, np.float64)) for b in range(B)])
    R_true = np.stack([_rot(g) for _ in range(B)])
    t_true = g.standard_normal((B, 3))
    M = np.diag([1.0, 1.0, -1.0]) if mirror else EYE
    y = np.stack([R_true[b] @ _small_rot(g.standard_normal(3), 0.02) @ M @ x[b] + t_true[b][:, None]
                  + 0.01 * g.standard_normal((3, 1)) + _null_noise(g, x[b], w[b], 0.01) for b in range(B)])
    for b in range(B):
        s = _ref(x[b], y[b], w[b])[4]
        if D[1] == 1 and D[2] == 1:
            assert s[0] - s[2] <= 1e-12 * s[0], s
        elif D[1] == 1:
            assert s[1] - s[2] <= 1e-12 * s[0] < s[0] - s[1], s
        else:
            assert 0.5e-9 < (s[1] - s[2]) / s[1] < 2e-9, s
        R, t, _ = OP.paper_pose(x[b], y[b], w[b], 1.0, fix)
        ygt = R_true[b] @ x[b] + t_true[b][:, None]
        assert np.abs(ygt - y[b]).min() > 1e-5 and np.abs(ygt - (R @ x[b] + t[:, None])).min() > 1e-5
        assert np.sign(np.linalg.det(R)) == (-1 if mirror else 1)
    f = lambda yy, ww: OP.deepvcp_loss_paper(x, yy, ww, R_true, t_true, 0.5, reflection_fix=fix)[0]
    want_y = _fd(lambda yy: f(yy, w), y)
    want_w = _fd(lambda ww: f(y, ww), w)
    gy = _T(y.transpose(0, 2, 1), cuda).requires_grad_()
    gw = _T(w, cuda).requires_grad_()
    loss, _, _ = dvcp.paper.deepVCP_loss_paper(_T(x.transpose(0, 2, 1), cuda), gy, gw, _T(R_true, cuda),
                                               _T(t_true[..., None], cuda), 0.5, reflection_fix=fix)
    loss.backward()
    assert abs(float(loss.detach()) - f(y, w)) <= 1e-9
    for what, got, want in (("d y", gy.grad.cpu().numpy(), want_y.transpose(0, 2, 1)), ("d w", gw.grad.cpu().numpy(), want_w)):
        scale = np.abs(want).max()
        err = np.abs(got - want).max()
        assert err <= 1e-6 * scale, (what, err, scale)


def test_backward_rank_deficient_is_finite(cuda):
    """Coplanar, collinear and identical-point rows: the loss is not smooth there, so only
    finiteness is asserted, for deepVCP_loss and for the paper loss (both reflection settings,
    with and without rejection).  The full-rank rows' gradients match a run without the degenerate
    rows (alpha = 1: the |mean| term couples the rows through its sign; the 1 / B of the mean is
    undone, so the match is to rounding, 1e-12 of the largest entry, not bit-wise)."""
    import dvcp
    g = np.random.default_rng(250)
    n = 24
    names, x, y = _degenerate_rows(g, n, 0.01)
    x, y = x[:5], y[:5]                                  # generic0, coplanar, collinear, identical, generic1
    B = len(x)
    R_true = np.stack([_rot(g) for _ in range(B)])
    t_true = g.standard_normal((B, 3, 1))
    w = g.random((B, n)) + 0.05
    keep = [0, 4]

    def pose_grad(rows, alpha):
        yg = _T(y[rows].transpose(0, 2, 1), cuda).requires_grad_()
        loss, R, t = dvcp.deepVCP_loss(_T(x[rows].transpose(0, 2, 1), cuda), yg, _T(R_true[rows], cuda),
                                       _T(t_true[rows], cuda), alpha)
        loss.backward()
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(R).all()) and bool(torch.isfinite(t).all())
        assert bool(torch.isfinite(yg.grad).all())
        return yg.grad.cpu().numpy() * len(rows)

    pose_grad(list(range(B)), 0.5)
    ga, gb = pose_grad(list(range(B)), 1.0)[keep], pose_grad(keep, 1.0)
    assert np.abs(ga - gb).max() <= 1e-12 * np.abs(gb).max()

    def paper_grad(rows, fix, ratio):
        yg = _T(y[rows].transpose(0, 2, 1), cuda).requires_grad_()
        wg = _T(w[rows], cuda).requires_grad_()
        loss, R, t = dvcp.paper.deepVCP_loss_paper(_T(x[rows].transpose(0, 2, 1), cuda), yg, wg, _T(R_true[rows], cuda),
                                                   _T(t_true[rows], cuda), 0.5, reflection_fix=fix, inlier_ratio=ratio)
        loss.backward()
        for a in (loss, R, t, yg.grad, wg.grad):
            assert bool(torch.isfinite(a).all())
        return yg.grad.cpu().numpy() * len(rows), wg.grad.cpu().numpy() * len(rows)

    for fix in (True, False):
        for ratio in (1.0, 0.8):
            (ya, wa), (yb, wb) = paper_grad(list(range(B)), fix, ratio), paper_grad(keep, fix, ratio)
            assert np.abs(ya[keep] - yb).max() <= 1e-12 * np.abs(yb).max()
            assert np.abs(wa[keep] - wb).max() <= 1e-12 * np.abs(wb).max()


# ---------------------------------------------------------------------------- (e) paper solve
@pytest.mark.parametrize("fix", [True, False])
def test_paper_pose_few_weights(cuda, fix):
    """Rows whose weights have exactly 1, 2 and 3 non-zero entries (weighted H of rank 0, 1, 2;
    dyadic points and weights, so the centroids are exact and H is rank-deficient in floating
    point too), a mirrored and a coplanar-and-mirrored set, between generic rows."""
    from dvcp import ops
    g = np.random.default_rng(260)
    n = 24
    x = np.stack([g.standard_normal((3, n)), _dyadic(g, (3, n)), _dyadic(g, (3, n)), _dyadic(g, (3, n)),
                  g.standard_normal((3, n)), _coplanar(g, n), g.standard_normal((3, n))])
    B = len(x)
    y = np.stack([_pair(g, x[b], 0.01) for b in range(B)])
    y[4] = np.diag([1.0, 1.0, -1.0]) @ x[4] + 0.01 * g.standard_normal((3, n))          # mirrored
    y[5] = _rot(g) @ np.diag([-1.0, 1.0, 1.0]) @ x[5] + 0.3                              # coplanar and mirrored
    w = g.random((B, n)) + 0.05
    for b, nz in ((1, [7]), (2, [3, 20]), (3, [0, 11, 23])):
        w[b] = 0.0
        w[b, nz] = [2.0, 0.5, 1.0][:len(nz)] if len(nz) != 2 else [1.0, 1.0]
    R, t = ops.paper_pose(_T(x, cuda), _T(y, cuda), _T(w, cuda), reflection_fix=fix)
    R, t = R.cpu().numpy(), t.cpu().numpy()
    for b in range(B):
        s = _check_pose(("few weights", b), R[b], t[b], x[b], y[b], w[b], fix=fix)
        if b in (1, 2, 3):
            assert s[b - 1] <= 1e-14 * max(s[0], TINY), (b, s)
            assert abs(np.linalg.det(R[b]) - 1) <= 1e-12
    assert np.array_equal(R[1], EYE)
    assert np.linalg.det(R[4]) * (1 if fix else -1) > 0
    assert np.linalg.det(R[5]) > 0                       # rank 2: the proper optimum, with or without the fix
    rows = [0, 6]
    Rn, tn = ops.paper_pose(_T(x[rows], cuda), _T(y[rows], cuda), _T(w[rows], cuda), reflection_fix=fix)
    assert np.array_equal(Rn.cpu().numpy(), R[rows]) and np.array_equal(tn.cpu().numpy(), t[rows])


@pytest.mark.parametrize("n,ratio", [(1024, 0.8), (1025, 1.0), (4000, 1.0)])
def test_paper_pose_sizes_vs_checker(cuda, n, ratio):
    """The rejection at its LDS limit n = 1024, and the single solve past it (no LDS arrays)."""
    from oracle import paper as OP
    from dvcp import ops
    g = np.random.default_rng(270 + n)
    B = 2
    x = g.standard_normal((B, 3, n))
    y = np.stack([_pair(g, x[b], 0.02) for b in range(B)])
    bad = g.choice(n, n // 6, replace=False)
    y[:, :, bad] += 2.0 * g.standard_normal((B, 3, len(bad)))
    w = g.random((B, n)) + 0.05
    R, t = ops.paper_pose(_T(x, cuda), _T(y, cuda), _T(w, cuda), inlier_ratio=ratio)
    for b in range(B):
        R_o, t_o, _ = OP.paper_pose(x[b], y[b], w[b], ratio)
        assert np.abs(R[b].cpu().numpy() - R_o).max() <= 1e-9 and np.abs(t[b].cpu().numpy()[:, 0] - t_o).max() <= 1e-9


def test_paper_pose_rejects_rejection_past_1024(cuda):
    from dvcp import ops
    x = torch.randn(2, 3, 1025, dtype=torch.float64, device=cuda)
    w = torch.rand(2, 1025, dtype=torch.float64, device=cuda) + 0.05
    with pytest.raises(RuntimeError, match="rejection needs 1 <= int"):
        ops.paper_pose(x, x + 0.5, w, inlier_ratio=0.8)
    torch.cuda.synchronize()


def test_paper_pose_all_zero_weights_row_is_nan(cuda):
    """A pair whose weights are all zero has no centroid (0 / 0): NaN for that pair only, every
    other pair bit-identical to a call without it (documented in include/dvcp.h)."""
    from dvcp import ops
    g = np.random.default_rng(280)
    B, n = 4, 64
    x = g.standard_normal((B, 3, n))
    y = np.stack([_pair(g, x[b], 0.02) for b in range(B)])
    w = g.random((B, n)) + 0.05
    w[2] = 0.0
    others = [0, 1, 3]
    for ratio in (1.0, 0.8):
        R, t = ops.paper_pose(_T(x, cuda), _T(y, cuda), _T(w, cuda), inlier_ratio=ratio)
        assert bool(torch.isnan(R[2]).all()) and bool(torch.isnan(t[2]).all())
        Rn, tn = ops.paper_pose(_T(x[others], cuda), _T(y[others], cuda), _T(w[others], cuda), inlier_ratio=ratio)
        assert torch.equal(R[others], Rn) and torch.equal(t[others], tn)
        assert bool(torch.isfinite(Rn).all())
