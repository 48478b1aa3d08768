"""CPU-side checks of the large-grid CPG path (dvcp_cpg_tiled): which forward a grid side takes
and the workspace size query."""
import pytest


def test_cpg_method_by_grid_side():
    from dvcp import ops
    for G in range(1, 12):
        assert ops.cpg_method(G) == "lds", G
    for G in range(12, 33):
        assert ops.cpg_method(G) == "tiled", G
    with pytest.raises(ValueError, match="32"):
        ops.cpg_method(33)


def test_gpu_test_grid_sides_are_exact():
    """The (r, s = 0.25) pairs tests/test_gpu_cpg_tiled.py takes its grids from: int(2r/s + 1) is
    exact in binary for each."""
    radii = {1: 0.0, 2: 0.125, 6: 0.625, 11: 1.25, 12: 1.375, 13: 1.5, 17: 2.0, 23: 2.75, 32: 3.875}
    for G, r in radii.items():
        assert int((2 * r) / 0.25 + 1) == G


def test_training_guard_names_the_limit():
    """The guard the autograd forward runs before any launch (no GPU needed to hit it)."""
    from dvcp import autograd
    autograd.require_trainable_grid(11)
    with pytest.raises(NotImplementedError, match="inference-only"):
        autograd.require_trainable_grid(12)


@pytest.mark.parametrize("G", [1, 11, 12, 13, 21, 32])
def test_cpg_tiled_workspace_bytes(G):
    """49 C floats per key point up to the chunk, constant beyond it (the entry point walks the key
    points in chunks), never above the 256 MiB cap; nothing for P = 0 or an unsupported grid."""
    import dvcp
    lib = dvcp.load_library()
    per = 49 * G ** 3 * 4
    sizes = [int(lib.dvcp_cpg_tiled_workspace_bytes(P, G)) for P in range(0, 4097)]
    assert sizes[0] >= 0
    assert sizes[1] == per
    assert all(s > 0 for s in sizes[1:])
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    chunk = sizes[-1] // per
    assert sizes[-1] == chunk * per and sizes[-1] <= 256 << 20
    for P in range(1, 4097):
        assert sizes[P] == min(P, chunk) * per, P
    big = int(lib.dvcp_cpg_tiled_workspace_bytes(1 << 21, G))
    assert big == int(lib.dvcp_cpg_tiled_workspace_bytes(1 << 22, G)) <= 256 << 20 and big >= sizes[-1]
    if G >= 11:     # the chunk is below 4096 key points: constant from there on
        assert big == sizes[-1] and chunk < 4096
    assert int(lib.dvcp_cpg_tiled_workspace_bytes(4, 33)) == 0


def test_cpg_tiled_rejects_bad_arguments():
    """Bad sizes and null pointers come back as errors before any launch."""
    import dvcp
    from dvcp import _lib
    dvcp.load_library()
    P8 = _lib.ctypes.c_void_p(16)
    with pytest.raises(RuntimeError, match="grid side G=33"):
        _lib.call("dvcp_cpg_tiled", P8, P8, 0, 0, 0, P8, 1, 33, P8, P8, None, P8, 1 << 30, None)
    with pytest.raises(RuntimeError, match="grid side G=0"):
        _lib.call("dvcp_cpg_tiled", P8, P8, 0, 0, 0, P8, 1, 0, P8, P8, None, P8, 1 << 30, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib.call("dvcp_cpg_tiled", None, P8, 0, 0, 0, P8, 1, 12, P8, P8, None, P8, 1 << 30, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib.call("dvcp_cpg_tiled", P8, P8, 0, 0, 0, P8, 1, 12, P8, P8, None, None, 1 << 30, None)
    with pytest.raises(RuntimeError, match="workspace"):
        _lib.call("dvcp_cpg_tiled", P8, P8, 0, 0, 0, P8, 1, 12, P8, P8, None, P8, 49 * 12 ** 3 * 4 - 4, None)
    with pytest.raises(RuntimeError, match="aligned"):
        _lib.call("dvcp_cpg_tiled", P8, P8, 0, 0, 0, P8, 1, 12, P8, P8, None, _lib.ctypes.c_void_p(8), 1 << 30, None)
    _lib.call("dvcp_cpg_tiled", None, None, 0, 0, 0, None, 0, 12, None, None, None, None, 0, None)   # P = 0: no-op
