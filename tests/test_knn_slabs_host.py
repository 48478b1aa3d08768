"""Host side of the slab kNN (dvcp_knn_slabs): the workspace size function and the slab geometry."""
import pytest


@pytest.fixture(scope="module")
def lib():
    import dvcp
    return dvcp.load_library()


def _bound(lib, B, M, Q, k):
    """The issue's ceiling: one full tiled workspace, one slab result plus the running keys, the
    packed points, 64 KiB of slack."""
    return lib.dvcp_knn_tiled_workspace_bytes(B, 16384, Q) + 16 * B * Q * k + 16 * B * M + 65536


def test_workspace_bytes_rejects_bad_arguments(lib):
    for args in ((-1, 100, 100, 8), (1, -1, 100, 8), (1, 100, -1, 8), (1, 100, 100, -1)):
        assert lib.dvcp_knn_slabs_workspace_bytes(*args) == -1, args
    assert lib.dvcp_knn_slabs_workspace_bytes(1, (1 << 20) + 1, 100, 8) == -1      # above the documented limit
    assert lib.dvcp_knn_slabs_workspace_bytes(1, 1 << 20, 100, 8) > 0


@pytest.mark.parametrize("B,M,Q,k", [(8, 65536, 85184, 32), (2, 16385, 130, 1)])
def test_workspace_bytes_within_bound(lib, B, M, Q, k):
    n = lib.dvcp_knn_slabs_workspace_bytes(B, M, Q, k)
    # what the call lays out: a slab's tiled workspace, its indices, the running keys, the points
    from dvcp import ops
    _, length = ops.knn_slab_geometry(M)
    least = lib.dvcp_knn_tiled_workspace_bytes(B, length, Q) + 12 * B * Q * k + 16 * B * M
    assert least <= n <= _bound(lib, B, M, Q, k), (n, least)


def test_workspace_does_not_grow_with_slab_count(lib):
    B, Q, k = 8, 85184, 32
    a = lib.dvcp_knn_slabs_workspace_bytes(B, 32768, Q, k)
    b = lib.dvcp_knn_slabs_workspace_bytes(B, 65536, Q, k)
    assert b - a == 16 * B * (65536 - 32768)
    c = lib.dvcp_knn_slabs_workspace_bytes(B, 1 << 20, Q, k)
    assert c - b == 16 * B * ((1 << 20) - 65536)


def test_slab_geometry_examples():
    from dvcp import ops

    def lengths(M):
        n, length = ops.knn_slab_geometry(M)
        return [min(length, M - j * length) for j in range(n)]

    assert lengths(16385) == [8208, 8177]
    assert lengths(32769) == [10928, 10928, 10913]
    assert lengths(65536) == [16384] * 4
    assert lengths(16384) == [16384] and lengths(5000) == [5000] and lengths(1) == [1]
    for M in (16385, 20000, 49153, 65535, 100000, 1 << 20):
        ls = lengths(M)
        assert sum(ls) == M and all(0 < x <= 16384 for x in ls) and ls[0] % 16 == 0, M
