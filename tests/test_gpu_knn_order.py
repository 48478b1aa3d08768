"""The tiled kNN's wave order (csrc/knn_tiled.hip, knn_wave_order): a certified bound B0 on the
32nd distance, tiles above it dropped, the rest counting-sorted into buckets of their lower bound,
and a scan that assumes no total order.  Results must equal the brute-force method bit for bit
whatever the order does; dvcp_knn_tiled_order_probe shows which case a wave ran."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KTILE = 16


def _equal_brute(ref, qry, k):
    from dvcp import ops
    d1, i1, _ = ops.knn(ref, qry, k, method="brute")
    d2, i2, i64 = ops.knn(ref, qry, k, method="tiled")
    assert torch.equal(i1, i2) and torch.equal(d1, d2)
    assert torch.equal(i64, i2.long())
    return d2, i2


def _probe(ref, qry):
    """dvcp_knn_tiled_order_probe on (B, M, 3) references and (B, Q, 3) queries: numpy arrays
    info (B, W, 4), order, lb, bucket (B, W, T) and the bound b0 (B, W)."""
    from dvcp import _lib
    B, M, _ = ref.shape
    Q = qry.shape[1]
    T, W = (M + KTILE - 1) // KTILE, (Q + 63) // 64
    dev = ref.device
    ws = torch.empty(int(_lib.load().dvcp_knn_tiled_workspace_bytes(B, M, Q)), dtype=torch.uint8, device=dev)
    info = torch.full((B, W, 4), -7, dtype=torch.int32, device=dev)
    order = torch.full((B, W, T), -7, dtype=torch.int32, device=dev)
    lb = torch.full((B, W, T), -7.0, dtype=torch.float32, device=dev)
    bucket = torch.full((B, W, T), -7, dtype=torch.int32, device=dev)
    rb, rn, rc = ref.stride()
    qb, qn, qc = qry.stride()
    _lib.call("dvcp_knn_tiled_order_probe", _lib.dtype_code(ref), _lib.ptr(ref), rb, rc, rn, M, _lib.ptr(qry), qb, qc,
              qn, Q, B, _lib.ptr(ws), _lib.ptr(info), _lib.ptr(order), _lib.ptr(lb), _lib.ptr(bucket), _lib.stream())
    torch.cuda.synchronize()
    info = info.cpu().numpy()
    b0 = info[..., 3].copy().view(np.float32)
    return info, order.cpu().numpy(), lb.cpu().numpy(), bucket.cpu().numpy(), b0


def _cube_inputs(M, Q, B, seed):
    """References in a rotated cube, queries in a box four times as wide around it (many outside),
    a third of them identical."""
    from dvcp.synthetic import rot_xyz
    g = torch.Generator().manual_seed(seed)
    ref = (torch.rand(B, M, 3, generator=g) * 2 - 1) @ torch.from_numpy(rot_xyz(0.4, 1.1, 2.0)).float().T + 0.7
    qry = torch.rand(B, Q, 3, generator=g) * 8 - 4
    qry[:, : Q // 3] = qry[:, :1]
    return ref, qry


# ------------------------------------------------------------------ 1. tile and certificate edges
@pytest.mark.parametrize("B", [1, 8])
@pytest.mark.parametrize("k", [17, 32])
@pytest.mark.parametrize("M", [20, 31, 32, 33, 512, 527, 1000, 10000, 16384])
def test_tile_and_certificate_edges(cuda, M, k, B):
    """Fewer than 32 references, exactly two tiles, a padded last tile (33, 527, 1000), every
    tile-count template (1, 2, 4, 8, 16 key registers); B = 8 takes the XCD cloud mapping.  Below
    32 references nothing may certify; two full tiles in reach of a compact wave must."""
    ref, qry = _cube_inputs(M, 2001, B, seed=1000 * M + B)
    ref, qry = ref.to(cuda), qry.to(cuda)
    _equal_brute(ref, qry, k)
    info, _, _, _, b0 = _probe(ref, qry)
    T = (M + KTILE - 1) // KTILE
    assert (info[..., 0] + info[..., 1] == T).all()
    if M < 32:
        assert (info[..., 2] == 0).all() and np.isinf(b0).all() and (info[..., 0] == 0).all()
    else:
        assert (info[..., 2] == 1).all() and np.isfinite(b0).all()  # finite queries, two full tiles


# --------------------------------------------------------------------------- 2. geometry sweep
_GEO_BLOCKS = ("cluster", "face", "far0.5", "far2", "far8", "far64", "far64_compact")
_GEO_Q = 1024
_FAR_WIDTH = 8.0


def _geometry_inputs():
    """One 10,000-point unit cube with a dense cluster, the same in every cloud; cloud i holds one
    query block: inside the cluster, on the cube's face x = 1, and 0.5, 2, 8, 64 cube widths off
    that face.

    The far blocks are 8 cube widths across, centred on the cube in y and z.  Whether a far wave
    can drop a tile is a matter of its own width, not of its distance: per axis, the far-corner
    extent to any tile is (gap to that tile) + (wave box width) + (tile width), and the gap to any
    other tile of the unit cube is at most one cube width larger, so once a wave's box is at least
    one cube width wide on every axis every tile's upper bound is at or above every tile's lower
    bound, B0 is too, and nothing can be dropped.  1024 queries in curve order make 16 waves of
    such a block, each about a sixteenth of its volume (4 x 4 x 2 cube widths): the case the far
    assertion is about.  A last block, a quarter of a cube width across and 64 widths away, is the
    opposite case: its waves see the cube's tiles at well separated distances and drop most."""
    g = torch.Generator().manual_seed(2024)
    cube = torch.rand(10000, 3, generator=g)
    centre = torch.tensor([0.3, 0.6, 0.4])
    cube[:3000] = centre + 0.02 * torch.randn(3000, 3, generator=g)
    cube = cube[torch.randperm(10000, generator=g)]
    blocks = [centre + 0.02 * torch.randn(_GEO_Q, 3, generator=g)]
    face = torch.rand(_GEO_Q, 3, generator=g)
    face[:, 0] = 1.0
    blocks.append(face)
    lateral = 0.5 - _FAR_WIDTH / 2
    for w in (0.5, 2.0, 8.0, 64.0):
        blk = torch.rand(_GEO_Q, 3, generator=g) * _FAR_WIDTH + torch.tensor([1.0 + w, lateral, lateral])
        blocks.append(blk)
    blocks.append(torch.rand(_GEO_Q, 3, generator=g) * 0.25 + torch.tensor([65.0, 0.4, 0.4]))
    return cube[None].repeat(len(blocks), 1, 1).contiguous(), torch.stack(blocks).contiguous()


@pytest.fixture(scope="module")
def geometry(cuda):
    ref, qry = _geometry_inputs()
    ref, qry = ref.to(cuda), qry.to(cuda)
    return ref, qry, _probe(ref, qry)


@pytest.mark.parametrize("k", [17, 32])
def test_geometry_sweep_equals_brute(cuda, geometry, k):
    ref, qry, _ = geometry
    _equal_brute(ref, qry, k)


def test_geometry_cluster_drops_tiles(geometry):
    """Queries inside the dense cluster: 32 points lie within a tiny certified bound, and most of
    the cube's 625 tiles are above it."""
    info = geometry[2][0]
    c = _GEO_BLOCKS.index("cluster")
    print("cluster: dropped per wave", info[c, :, 0].tolist())
    assert (info[c, :, 2] == 1).all()
    assert (info[c, :, 0] > 0).all()


def test_geometry_far_block_finite_bound_drops_nearly_none(geometry):
    """64 cube widths away: a finite B0, and none or nearly none of the tiles dropped (at most one
    in sixteen; none at all wherever a wave's box is a cube width wide on every axis, see
    _geometry_inputs).  The order then has every tile in the top buckets of a finite bound."""
    info, _, _, _, b0 = geometry[2]
    f = _GEO_BLOCKS.index("far64")
    T = info[f, 0, 0] + info[f, 0, 1]
    print("far64: B0 per wave", b0[f].tolist())
    print("far64: dropped per wave of", T, "tiles:", info[f, :, 0].tolist())
    assert (info[f, :, 2] == 1).all() and np.isfinite(b0[f]).all()
    assert (info[f, :, 0] <= T // 16).all()


def test_geometry_far_compact_block_drops_far_tiles(geometry):
    """A block a quarter of a cube width across, 64 widths away: B0, the far corner of the second
    nearest tile, is about (65.25 - 0.9)^2 plus the lateral terms, and a tile whose near face lies
    more than about 0.4 further off has a lower bound above it: more than half of the cube's tiles
    are provably beyond every query's 32nd distance and must be dropped."""
    info, _, _, _, b0 = geometry[2]
    f = _GEO_BLOCKS.index("far64_compact")
    T = info[f, 0, 0] + info[f, 0, 1]
    print("far64_compact: B0 per wave", b0[f].tolist())
    print("far64_compact: dropped per wave of", T, "tiles:", info[f, :, 0].tolist())
    assert (info[f, :, 2] == 1).all() and np.isfinite(b0[f]).all()
    assert (info[f, :, 0] > T // 2).all()


# --------------------------------------------------------------------- 3. ties across the bound
@pytest.mark.parametrize("k", [32, 20])
def test_ties_across_the_bound(cuda, k):
    """References on a 1/8 grid with about 2.4 copies of every grid point, shuffled: the copies of
    a point share a curve cell, so groups of equal distances at the 32nd/33rd key straddle tiles
    and buckets.  Queries on grid points and on midpoints; the order must be (d2, index)."""
    g = torch.Generator().manual_seed(31)
    ref = (torch.randint(-8, 9, (2, 12000, 3), generator=g).float() / 8)
    on = torch.randint(-10, 11, (2, 1500, 3), generator=g).float() / 8
    mid = torch.randint(-10, 10, (2, 1500, 3), generator=g).float() / 8 + 1.0 / 16
    qry = torch.cat([on, mid], 1)
    _equal_brute(ref.to(cuda), qry.to(cuda), k)


# ------------------------------------------------------------------------ 4. degenerate ranges
def test_all_references_equal(cuda):
    """Every reference the same point.  Cloud 0: every query equal to it (B0 = 0, a zero bucket
    range); cloud 1: queries elsewhere, some equal."""
    p = torch.tensor([0.25, -1.5, 3.0])
    ref = p.expand(2, 1000, 3).contiguous()
    g = torch.Generator().manual_seed(5)
    qry = torch.stack([p.expand(640, 3), torch.rand(640, 3, generator=g) * 6 - 3])
    qry[1, ::7] = p
    ref, qry = ref.to(cuda), qry.contiguous().to(cuda)
    for k in (17, 32):
        d, i = _equal_brute(ref, qry, k)
        assert (d[0] == 0).all() and torch.equal(i[0, 0].cpu(), torch.arange(k, dtype=torch.int32))
    info, _, _, _, b0 = _probe(ref, qry)
    assert (b0[0] == 0).all() and (info[0, :, 2] == 1).all()


def test_mostly_infinite_references(cuda):
    """490 of 512 references at +inf: 22 finite keys, then (inf, -1); nothing certifies."""
    g = torch.Generator().manual_seed(6)
    ref = torch.rand(2, 512, 3, generator=g)
    for b in range(2):
        ref[b, torch.randperm(512, generator=g)[:490]] = float("inf")
    qry = torch.rand(2, 700, 3, generator=g) * 2 - 0.5
    ref, qry = ref.to(cuda), qry.to(cuda)
    for k in (17, 32):
        d, i = _equal_brute(ref, qry, k)
        assert (i[..., :17] >= 0).all() and torch.isfinite(d[..., :17]).all()
        if k == 32:
            assert (i[..., 22:] == -1).all() and torch.isinf(d[..., 22:]).all() and (i[..., :22] >= 0).all()
    info = _probe(ref, qry)[0]
    assert (info[..., 2] == 0).all() and (info[..., 0] == 0).all()


def test_nan_query_row(cuda):
    """One NaN query among finite ones: its row is (inf, -1); its wave certifies nothing, and the
    other rows are unaffected."""
    ref, qry = _cube_inputs(4000, 1000, 2, seed=77)
    qry[0, 333] = float("nan")
    qry[1, 64, 1] = float("nan")
    ref, qry = ref.to(cuda), qry.to(cuda)
    d, i = _equal_brute(ref, qry, 32)
    assert (i[0, 333] == -1).all() and torch.isinf(d[0, 333]).all()
    info = _probe(ref, qry)[0]
    assert (info[0, :, 2] == 0).sum() == 1 and (info[1, :, 2] == 0).sum() == 1


@pytest.mark.parametrize("Q", [65, 64 * 9 + 1])
def test_ragged_last_wave(cuda, Q):
    """Q = 64 n + 1: the last wave has one live lane, and its box is that query alone."""
    ref, qry = _cube_inputs(5000, Q, 3, seed=Q)
    _equal_brute(ref.to(cuda), qry.to(cuda), 32)
    _equal_brute(ref.to(cuda), qry.to(cuda), 17)


# --------------------------------------------------------------------------- 5. large magnitudes
@pytest.mark.parametrize("k", [17, 32])
def test_large_magnitudes(cuda, k):
    """Coordinates near 1e4 on a 1e-2 lattice (fp32 spacing there is 1e-3, so the roundings of d2
    are comparable to the gaps between neighbours, and the half-precision boxes are 8 wide): the
    certificate's bound must still lie above every computed distance."""
    g = torch.Generator().manual_seed(9)
    ref = 1e4 + torch.randint(0, 200, (2, 6000, 3), generator=g).float() * 1e-2
    qry = 1e4 + torch.randint(-50, 250, (2, 2000, 3), generator=g).float() * 1e-2 + 5e-3
    qry[1] = qry[1] + torch.tensor([40.0, 0.0, -25.0])       # a block well outside the cloud
    _equal_brute(ref.to(cuda), qry.to(cuda), k)


# --------------------------------------------------------------------------- 6. probe consistency
def test_probe_order_is_consistent(geometry):
    """For every wave of the geometry sweep: the order is a permutation of the tiles whose lower
    bound does not exceed B0, and the buckets do not decrease along it."""
    info, order, lb, bucket, b0 = geometry[2]
    B, W, T = order.shape
    for b in range(B):
        for w in range(W):
            dropped, kept = int(info[b, w, 0]), int(info[b, w, 1])
            assert dropped + kept == T
            keep = ~(lb[b, w] > b0[b, w])
            ids = order[b, w, :kept]
            assert (order[b, w, kept:] == -1).all()
            assert np.array_equal(np.sort(ids), np.flatnonzero(keep)), (b, w)
            assert ((bucket[b, w] == -1) == ~keep).all()
            along = bucket[b, w, ids]
            assert (along >= 0).all() and (np.diff(along) >= 0).all(), (b, w)
            assert (lb[b, w] >= 0).all()
