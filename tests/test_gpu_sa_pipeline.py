"""The set-abstraction table kernels (csrc/sa_mfma_sa1.hip, _sa2.hip, _sa3.hip) walk each wave's centres as one flat
tile sequence and prefetch: the list entry of tile t + 2 and the gathered U row / point of tile
t + 1 are in flight while tile t runs.  These tests pin what such a pipeline can get wrong: a tile
fed another tile's gathered rows, centre or running maximum, a prefetch through the list row of a
centre without hits, and the pipeline's drain and re-prime at the 64-centre batch boundary.

Lists are built by hand.  Counts cycle through COUNTS (capped at nsample) along the flat centre
index, period 11, so centres without hits sit between centres with hits; the wave strides
(16384 centres flat, 2048 per XCD) are no multiple of 11, so among the waves that walk two
centres every (first, last) pair of counts occurs, the pairs with an empty first and an empty
last centre included (for sa1 at B = 3: wave 0 holds centres 0 and 16384 with counts (0, 31),
wave 6 centres 6 and 16390 with counts (32, 0); sa2 / sa3 visit their centres in curve order, so
there which wave gets which pair depends on the coordinates).  List rows of centres without hits
hold 1 << 30, every other entry a random valid index (with repeats).  The clouds lie in a cube of
the ball's radius, so the local coordinates are of the size a ball query's output gives."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, None)  # None: the table's nsample
SHAPES = {"xcd": (8, 2100, 2100), "flat": (3, 5600, 5600)}  # B % 8 == 0: XCD mapping; else flat
BOUNDARY = (8, 140000, 64, 2)  # B, S, N, nsample: 68 centres per wave, so a second 64-centre batch


def _make(table, B, S, N, ns, rows_variant, seed):
    """Model pair and hand-built inputs (CPU) for one table."""
    import dvcp.pointnet2_utils as P
    import oracle as O
    from tests_helpers import randomize_bn
    cfg = O.fe_config(use_normal=False, npoint=S)[table]
    ns = min(cfg["nsample"], N) if ns is None else ns
    D = cfg["in_channel"] - 3
    torch.manual_seed(17 + table)
    ref = O.PointNetSetAbstraction(**cfg).eval()
    randomize_bn(ref)
    mine = P.PointNetSetAbstraction(**cfg).eval()
    mine.load_state_dict(ref.state_dict())
    g = torch.Generator().manual_seed(seed)
    r = cfg["radius"]
    xyz = ((torch.rand(B, 3, N, generator=g, dtype=torch.float64) - 0.5) * r).float()
    ctr = ((torch.rand(B, 3, S, generator=g, dtype=torch.float64) - 0.5) * r).float()
    vals = torch.tensor([ns if v is None else min(v, ns) for v in COUNTS], dtype=torch.int32)
    count = vals[torch.arange(B * S) % len(COUNTS)].view(B, S).contiguous()
    lst = torch.randint(0, N, (B, S, ns), generator=g, dtype=torch.int32)
    lst[count == 0] = 1 << 30
    feat = rows = None
    if D:
        if rows_variant:  # point n takes feature row rows[b, n]: repeated and out of order
            Nf = N // 2 + 3
            feat = torch.randn(B, Nf, D, generator=g)
            rows = torch.randint(0, Nf, (B, N), generator=g)
        else:
            feat = torch.randn(B, N, D, generator=g)
    return dict(ref=ref, mine=mine, ns=ns, xyz=xyz, ctr=ctr, count=count, lst=lst, feat=feat, rows=rows)


def _run(c, dev, perm=None):
    """The table on the GPU, centres optionally permuted (ctr, count and lst together)."""
    from dvcp import ops
    mine = c["mine"].to(dev)
    ctr, count, lst = c["ctr"], c["count"], c["lst"]
    if perm is not None:
        ctr, count, lst = ctr[:, :, perm].contiguous(), count[:, perm].contiguous(), lst[:, perm].contiguous()
    xyz, ctr, count, lst = c["xyz"].to(dev), ctr.to(dev), count.to(dev), lst.to(dev)
    if c["rows"] is not None:
        out = ops.sa_group_mlp_rows(xyz, ctr, c["feat"].to(dev), c["rows"].to(dev), count, lst, c["ns"], mine.chans,
                                    mine.packed_params())
    else:
        feat = c["feat"].to(dev).transpose(1, 2) if c["feat"] is not None else None
        out = ops.sa_group_mlp(xyz, ctr, feat, count, lst, c["ns"], mine.chans, mine.packed_params(), xyz_pdim=2,
                               feat_ddim=1, feat_pdim=2)
    torch.cuda.synchronize()
    return out.cpu()


def _oracle(c):
    """The oracle's grouped MLP on the same lists: gather with padding by the first hit
    (pointnet2_utils.py:104-106), local coordinates, [conv, BN, ReLU]*, max over the rows."""
    import oracle as O
    ref, ns = c["ref"], c["ns"]
    col = torch.arange(ns)
    outs = []
    with torch.no_grad():
        for b in range(c["xyz"].shape[0]):
            cnt = c["count"][b].long()
            lb = c["lst"][b].long()
            gidx = torch.where(col[None, :] < cnt[:, None], lb, lb[:, :1])
            gidx[cnt < 1] = 0  # centres without hits: not compared (the kernels give zeros)
            pts = c["xyz"][b].t()[None]                          # (1, N, 3)
            grouped = O.index_points(pts, gidx[None]) - c["ctr"][b].t()[None, :, None, :]
            if c["feat"] is not None:
                f = c["feat"][b] if c["rows"] is None else c["feat"][b][c["rows"][b]]
                grouped = torch.cat([grouped, O.index_points(f[None], gidx[None])], dim=-1)
            x = grouped.permute(0, 3, 2, 1)                      # (1, C0, ns, S)
            for conv, bn in zip(ref.mlp_convs, ref.mlp_bns):
                x = torch.nn.functional.relu(bn(conv(x.float())))
            outs.append(torch.max(x, 2)[0].permute(0, 2, 1))    # (1, S, C)
    return torch.cat(outs)


@functools.lru_cache(maxsize=None)
def _case(table, shape):
    """Inputs, the GPU table and the oracle's, computed once per (table, shape)."""
    B, S, N = SHAPES[shape]
    c = _make(table, B, S, N, None, rows_variant=(table == 2), seed=500 + 10 * table + B)
    c["got"] = _run(c, torch.device("cuda:0"))
    return c


def _check_position_independent(c, got, dev, seed):
    S = c["ctr"].shape[2]
    perm = torch.randperm(S, generator=torch.Generator().manual_seed(seed))
    again = _run(c, dev, perm)
    assert torch.equal(again, got[:, perm])


def _check_oracle(c, got):
    want = _oracle(c)
    empty = c["count"] < 1
    assert torch.equal(got[empty], torch.zeros_like(got[empty]))
    torch.testing.assert_close(got[~empty], want[~empty], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("table", [0, 1, 2])
def test_sa_pipeline_position_independent(cuda, table, shape):
    """The same centres in a permuted order give bit-identical rows: sa1 and sa2 through
    ops.sa_group_mlp, sa3 through ops.sa_group_mlp_rows with repeated, out-of-order rows."""
    c = _case(table, shape)
    _check_position_independent(c, c["got"], cuda, seed=9 + table)


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("table", [0, 1, 2])
def test_sa_pipeline_vs_oracle(cuda, table, shape):
    """Every centre with hits matches the oracle's grouped MLP on the same lists (the tolerances of
    test_set_abstraction_vs_oracle); every centre without hits is exactly zero."""
    c = _case(table, shape)
    _check_oracle(c, c["got"])


@pytest.mark.parametrize("table", [0, 1, 2])
def test_sa_pipeline_batch_boundary(cuda, table):
    """More than 64 x 16384 centres with nsample 2: every wave's 64-centre batch loop runs a second
    time, so the pipeline drains and is primed again inside one wave.  Both checks."""
    B, S, N, ns = BOUNDARY
    c = _make(table, B, S, N, ns, rows_variant=(table == 2), seed=900 + table)
    got = _run(c, cuda)
    _check_position_independent(c, got, cuda, seed=31 + table)
    _check_oracle(c, got)
