"""kNN above 16384 reference points (dvcp_knn_slabs, ops.knn method "tiled_slabs"): the reference
cut into index slabs, the tiled kernels per slab, and a fold ordered by (d2, global index).  Every
result is bit-equal to the brute-force kernel (dvcp_knn), which scans in index order and shares no
code with the slab path."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _inputs(cuda, M, Q, B, seed):
    """test_gpu_kernels._c3_knn_inputs: FE-like references, queries partly far outside the cloud,
    duplicated points; here a second block of duplicates 20000 indices apart, in another slab."""
    from dvcp.synthetic import rot_xyz
    g = torch.Generator().manual_seed(seed)
    ref = (torch.rand(B, M, 3, generator=g) * 2 - 1)
    ref = ref @ torch.from_numpy(rot_xyz(0.4, 1.1, 2.0)).float().T + 0.7
    if M >= 5100:
        ref[:, 5000:5100] = ref[:, 100:200]
    if M >= 20100:
        ref[:, 20000:20100] = ref[:, 100:200]                 # ties across slabs -> the lower slab
    qry = torch.rand(B, Q, 3, generator=g) * 8 - 4
    qry[:, :40] = ref[:, 100:140]                              # queries on the duplicated points
    return ref.to(cuda), qry.to(cuda)


def _same(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("k", [1, 16, 17, 32])
@pytest.mark.parametrize("M", [16385, 16400, 32768, 32769, 65536, 100000])
def test_knn_slabs_edges_equal_brute(cuda, M, k):
    """2, 3, 4 and 7 slabs, a short last slab, a ragged query wave, both list lengths of the fold
    (k <= 16, k > 16): dist, idx and idx64 bit-equal to brute force."""
    from dvcp import ops
    ref, qry = _inputs(cuda, M, 130, 2, seed=M + k)
    want = ops.knn(ref, qry, k, method="brute")
    got = ops.knn(ref, qry, k, method="tiled_slabs")
    _same(got, want)
    assert got[1].dtype == torch.int32 and got[2].dtype == torch.int64
    if M >= 20100:
        # query j < 40 sits on reference 100 + j and its two copies: indices ascending at distance 0
        top = got[1][:, :40, :min(k, 3)].cpu()
        cols = torch.arange(100, 140)[None, :, None] + torch.tensor([0, 4900, 19900])[:min(k, 3)]
        assert torch.equal(top.long(), cols.expand(2, -1, -1))


def test_knn_slabs_automatic_dispatch(cuda):
    from dvcp import ops
    assert ops.knn_method(20000) == "tiled_slabs" and ops.knn_method(16385) == "tiled_slabs"
    assert ops.knn_method(16384) == "tiled" and ops.knn_method(100) == "brute"
    ref, qry = _inputs(cuda, 20000, 130, 2, seed=7)
    _same(ops.knn(ref, qry, 32), ops.knn(ref, qry, 32, method="brute"))


def test_knn_slabs_one_slab_forced(cuda):
    from dvcp import ops
    ref, qry = _inputs(cuda, 5000, 900, 2, seed=8)
    _same(ops.knn(ref, qry, 17, method="tiled_slabs"), ops.knn(ref, qry, 17, method="tiled"))
    # fewer references than k: the slab's padding entries stay last and come out as (inf, -1)
    d, i, i64 = ops.knn(ref[:, :20], qry, 32, method="tiled_slabs")
    _same((d, i, i64), ops.knn(ref[:, :20], qry, 32, method="brute"))
    assert bool((i[..., 20:] == -1).all()) and bool(torch.isinf(d[..., 20:]).all()) and bool((i[..., :20] >= 0).all())


@pytest.mark.parametrize("k", [2, 32])
def test_knn_slabs_sqrt_collision(cuda, k):
    """d2 = 1 (index 19000) and d2 = 1 + 2^-23 (index 5) both have dist 1.0f: the order is by d2, so
    the farther-indexed point comes first.  A fold ordered by (dist, index) returns [5, 19000]."""
    from dvcp import ops
    g = torch.Generator().manual_seed(9)
    M = 20000
    v = torch.randn(1, M, 3, generator=g)
    ref = v / v.norm(dim=-1, keepdim=True) * (3.05 + 2.0 * torch.rand(1, M, 1, generator=g))  # norm >= 3
    ref[0, 5] = torch.tensor([2.0 ** -12, 2.0 ** -12, 1.0])
    ref[0, 19000] = torch.tensor([0.0, 0.0, 1.0])
    assert float((ref[0, 5] ** 2).sum()) > 1.0 and float((ref[0, 5] ** 2).sum().sqrt()) == 1.0
    qry = torch.cat([torch.zeros(1, 1, 3), torch.rand(1, 64, 3, generator=g) * 8 - 4], dim=1)
    ref, qry = ref.to(cuda), qry.to(cuda)
    got = ops.knn(ref, qry, k, method="tiled_slabs")
    _same(got, ops.knn(ref, qry, k, method="brute"))
    assert got[1][0, 0, :2].tolist() == [19000, 5] and got[0][0, 0, :2].tolist() == [1.0, 1.0]


@pytest.mark.parametrize("k", [20, 32])
def test_knn_slabs_dyadic_ties(cuda, k):
    """Coordinates on a 1/8 grid: nearly every distance is tied, across three slabs."""
    from dvcp import ops
    g = torch.Generator().manual_seed(10 + k)
    ref = (torch.randint(-16, 17, (2, 40000, 3), generator=g).float() / 8).to(cuda)
    qry = (torch.randint(-16, 17, (2, 3000, 3), generator=g).float() / 8).to(cuda)
    _same(ops.knn(ref, qry, k, method="tiled_slabs"), ops.knn(ref, qry, k, method="brute"))


def test_knn_slabs_vs_oracle_fp64(cuda):
    """dvcp.KNN (automatic dispatch) on fp64 inputs, the cast path, against the oracle's KNN."""
    import oracle as O
    from dvcp.knn import KNN
    g = torch.Generator().manual_seed(11)
    ref = torch.rand(1, 20000, 3, generator=g, dtype=torch.float64) * 2 - 1
    qry = torch.rand(1, 600, 3, generator=g, dtype=torch.float64) * 3 - 1.5
    dw, iw = O.KNN(k=32, transpose_mode=True)(ref, qry)
    d, i = KNN(k=32, transpose_mode=True)(ref.to(cuda), qry.to(cuda))
    assert torch.equal(i.cpu(), iw) and torch.equal(d.cpu(), dw)


def test_knn_slabs_ignores_workspace_garbage(cuda):
    """The workspace needs no initialisation: the block the allocator hands back is filled with two
    different byte patterns before two calls on the same inputs."""
    from dvcp import _lib, ops
    ref, qry = _inputs(cuda, 33000, 500, 2, seed=12)
    n = int(_lib.load().dvcp_knn_slabs_workspace_bytes(2, 33000, 500, 32))
    outs = []
    for fill in (0xFF, 0x5A):
        junk = torch.empty(n, dtype=torch.uint8, device=cuda).fill_(fill)
        del junk                                               # the next torch.empty(n) reuses this block
        outs.append(ops.knn(ref, qry, 32, method="tiled_slabs"))
    _same(outs[0], outs[1])
    _same(outs[0], ops.knn(ref, qry, 32, method="brute"))
