"""CPU-side checks of the large-grid CPG backward (dvcp_cpg_tiled_backward): the opt-in training
guard, the workspace size query, the argument checks that come back before any launch, and that the
opt-in flag leaves the state_dict alone."""
import pytest

NPARAMS = 15681
CAP = 256 << 20


def _blocks(G):
    return (-(-G // 8)) ** 3   # per axis ceil(G / 8) blocks of at most 8 cells


def _per_point(G):
    """Bytes of the chunk region per key point: 74 C floats (the forward's 49 C, h2, dL/dlg, dL/dh2,
    dL/dh1) plus each block's partial sums (15681 parameters and 32 of d src) and db3, rounded up
    to 16 bytes."""
    floats = 74 * G ** 3 + _blocks(G) * (NPARAMS + 32) + 1
    return (floats + 3) // 4 * 16


def _partials(P):
    return (P * NPARAMS + 3) // 4 * 16


def test_training_guard_is_opt_in():
    from dvcp import autograd
    autograd.require_trainable_grid(11)
    autograd.require_trainable_grid(11, large_grid=True)
    with pytest.raises(NotImplementedError, match="inference-only"):
        autograd.require_trainable_grid(12)
    with pytest.raises(NotImplementedError, match="inference-only"):
        autograd.require_trainable_grid(12, large_grid=False)
    autograd.require_trainable_grid(12, large_grid=True)
    autograd.require_trainable_grid(32, large_grid=True)
    with pytest.raises(ValueError, match="G <= 32"):
        autograd.require_trainable_grid(33, large_grid=True)
    with pytest.raises(ValueError, match="G <= 32"):
        autograd.require_trainable_grid(33)


def test_cpg_tiled_backward_workspace_bytes():
    """Nothing for P <= 0 or an unsupported grid; one key point covered at every G; monotone in P;
    the partial sums of all P key points plus a chunk region under the 256 MiB cap."""
    import dvcp
    size = dvcp.load_library().dvcp_cpg_tiled_backward_workspace_bytes
    for G in (0, 33, -1):
        assert int(size(4, G)) == 0
    for G in range(1, 33):
        assert int(size(0, G)) == 0 and int(size(-3, G)) == 0
        assert int(size(1, G)) == _partials(1) + _per_point(G), G
        assert int(size(1, G)) % 16 == 0
    for G in (1, 11, 12, 13, 21, 32):
        per = _per_point(G)
        sizes = [int(size(P, G)) for P in range(1, 600)]
        assert all(b > a for a, b in zip(sizes, sizes[1:])), G   # the partials grow with every key point
        for P in (1, 2, 19, 20, 147, 599, 4096):
            chunk = int(size(P, G)) - _partials(P)
            assert chunk == min(P, CAP // per) * per, (G, P)
            assert per <= chunk <= CAP
    chunk = int(size(4096, 32)) - _partials(4096)
    assert 0 < chunk <= CAP and chunk % _per_point(32) == 0


def test_cpg_tiled_backward_rejects_bad_arguments():
    """Bad sizes, null pointers, a misaligned or too small workspace: errors before any launch."""
    import dvcp
    from dvcp import _lib
    dvcp.load_library()
    P8 = _lib.ctypes.c_void_p(16)

    def call(G=12, src=P8, ws=P8, ws_bytes=1 << 30, gp=P8):
        _lib.call("dvcp_cpg_tiled_backward", src, P8, 0, 0, 0, P8, 1, G, P8, P8, P8, P8, ws, ws_bytes, gp, None)

    with pytest.raises(RuntimeError, match="grid side G=33"):
        call(G=33)
    with pytest.raises(RuntimeError, match="grid side G=0"):
        call(G=0)
    with pytest.raises(RuntimeError, match="null pointer"):
        call(src=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        call(ws=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        call(gp=None)
    with pytest.raises(RuntimeError, match="aligned"):
        call(ws=_lib.ctypes.c_void_p(8))
    with pytest.raises(RuntimeError, match="workspace"):
        call(ws_bytes=_partials(1) + _per_point(12) - 4)
    with pytest.raises(RuntimeError, match="workspace"):
        call(ws_bytes=0)


def test_flag_leaves_state_dict_alone():
    import dvcp
    a, b = dvcp.cpg(), dvcp.cpg(train_large_grid=True)
    assert not a.train_large_grid and b.train_large_grid
    assert list(a.state_dict()) == list(b.state_dict())
    m0 = dvcp.DeepVCP(use_normal=False)
    m1 = dvcp.DeepVCP(use_normal=False, train_large_grid=True)
    assert not m0.cpg.train_large_grid and m1.cpg.train_large_grid
    assert list(m0.state_dict()) == list(m1.state_dict())
    assert not any("train_large_grid" in k for k in m1.state_dict())
    m0.load_state_dict(m1.state_dict())
