"""CPU-side checks of the split key-point stage (dvcp_src_keypoints_ws, K up to 1024): which stage a
key-point count takes, the workspace size query and the entry points' refusals before any launch."""
import pytest


def test_src_keypoints_method_by_k():
    from dvcp import ops
    assert ops.SRC_KEYPOINTS_LDS_MAX_K == 256 and ops.SRC_KEYPOINTS_MAX_K == 1024
    assert ops.src_keypoints_method(1) == "lds"
    assert ops.src_keypoints_method(256) == "lds"
    assert ops.src_keypoints_method(257) == "split"
    assert ops.src_keypoints_method(1024) == "split"
    with pytest.raises(ValueError, match="1024"):
        ops.src_keypoints_method(1025)


def test_workspace_bytes():
    """Positive multiples of 16 that hold the coordinates, the FPS order and the ball lists, growing
    with B and K; 0 for what the entry point refuses."""
    import dvcp
    lib = dvcp.load_library()
    q = lib.dvcp_src_keypoints_workspace_bytes
    for dtype, es in ((0, 4), (1, 8)):
        for ns in (1, 16, 32):
            for B in (1, 2, 3, 7):
                prev = 0
                for K in range(ns, 1025):
                    n = int(q(dtype, B, K, ns))
                    assert n > 0 and n % 16 == 0, (dtype, B, K, ns, n)
                    assert n >= B * (3 * K * es + 4 * K + 4 * K * ns), (dtype, B, K, ns, n)
                    assert n >= prev, (dtype, B, K, ns)
                    prev = n
        for K in (1, 33, 257, 1024):
            ns = min(K, 32)
            sizes = [int(q(dtype, B, K, ns)) for B in range(1, 66)]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (dtype, K)
    assert int(q(0, 2, 0, 1)) == 0
    assert int(q(0, 2, 1025, 32)) == 0
    assert int(q(0, 2, 64, 33)) == 0
    assert int(q(0, 2, 16, 32)) == 0     # K < nsample
    assert int(q(2, 2, 64, 32)) == 0     # bad dtype
    assert int(q(0, 0, 64, 32)) == 0


def test_ws_entries_reject_bad_arguments():
    """Bad sizes, a bad dtype and a bad workspace come back as errors before any launch."""
    import dvcp
    from dvcp import _lib
    lib = dvcp.load_library()
    P = _lib.ctypes.c_void_p(16)
    S, B, K, ns = 2000, 2, 512, 32
    need = int(lib.dvcp_src_keypoints_workspace_bytes(0, B, K, ns))

    def fwd(dtype=0, S=S, B=B, K=K, ns=ns, ws=P, nbytes=1 << 30, feat=P):
        _lib.call("dvcp_src_keypoints_ws", dtype, P, feat, S, P, B, K, P, 1.0, ns, P, 0, P, P, P, ws, nbytes, None)

    def bwd(dtype=0, S=S, B=B, K=K, ns=ns, ws=P, nbytes=1 << 30):
        _lib.call("dvcp_src_keypoints_backward_ws", dtype, ws, nbytes, S, B, K, ns, P, P, None)

    for f in (fwd, bwd):
        with pytest.raises(RuntimeError, match="null workspace"):
            f(ws=None)
        with pytest.raises(RuntimeError, match="workspace must be 16-byte aligned"):
            f(ws=_lib.ctypes.c_void_p(24))
        with pytest.raises(RuntimeError, match=f"workspace of {need - 1} bytes, need {need}"):
            f(nbytes=need - 1)
        with pytest.raises(RuntimeError, match="K=1025"):
            f(K=1025)
        with pytest.raises(RuntimeError, match="K=512.*S=511"):
            f(S=511)
        with pytest.raises(RuntimeError, match="nsample=33"):
            f(ns=33)
        with pytest.raises(RuntimeError, match="bad dtype 2"):
            f(dtype=2)
    with pytest.raises(RuntimeError, match="K=16 < nsample=32"):
        fwd(K=16)
    with pytest.raises(RuntimeError, match="K=16 nsample=32 unsupported"):
        bwd(K=16)
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib.call("dvcp_src_keypoints_ws", 0, None, P, S, P, B, K, P, 1.0, ns, P, 0, P, P, P, P, 1 << 30, None)
    with pytest.raises(RuntimeError, match="fe_feat must be 16-byte aligned"):
        fwd(feat=_lib.ctypes.c_void_p(8))
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib.call("dvcp_src_keypoints_backward_ws", 0, P, 1 << 30, S, B, K, ns, None, P, None)
    # B = 0: a no-op whatever the pointers
    _lib.call("dvcp_src_keypoints_ws", 0, None, None, S, None, 0, K, None, 1.0, ns, None, 0, None, None, None, None, 0,
              None)
    _lib.call("dvcp_src_keypoints_backward_ws", 0, None, 0, S, 0, K, ns, None, None, None)


def test_lds_entries_name_the_ws_entries():
    """The one-workgroup entries still stop at 256 key points and say where larger counts go."""
    import dvcp
    from dvcp import _lib
    dvcp.load_library()
    P = _lib.ctypes.c_void_p(16)
    with pytest.raises(RuntimeError, match=r"K=257 unsupported.*dvcp_src_keypoints_ws"):
        _lib.call("dvcp_src_keypoints", 0, P, P, 2000, P, 1, 257, P, 1.0, 32, P, 0, P, P, P, None)
    with pytest.raises(RuntimeError, match=r"K=257 nsample=32 unsupported.*dvcp_src_keypoints_backward_ws"):
        _lib.call("dvcp_src_keypoints_backward", 0, P, 2000, P, 1, 257, P, 1.0, 32, P, P, None)


def test_abi_version_unchanged():
    import dvcp
    assert dvcp.load_library().dvcp_abi_version() == 5


def test_k_limit_raises_before_any_op():
    """ops.src_keypoints and DeepVCP.forward refuse K = 1025 with the limit in the message before they
    touch a tensor (no GPU needed to get there); the constructor takes it, with the same state_dict."""
    import torch

    import dvcp
    from dvcp import ops
    big, small = dvcp.DeepVCP(use_normal=False, K=1025, fe_npoint=16), dvcp.DeepVCP(use_normal=False, K=64, fe_npoint=16)
    assert list(big.state_dict().keys()) == list(small.state_dict().keys())
    x = torch.rand(1, 3, 64)
    with pytest.raises(ValueError, match="1024"):
        big(x, x, torch.eye(3, dtype=torch.float64)[None], torch.zeros(1, 3))
    with pytest.raises(ValueError, match="1024"):
        ops.src_keypoints(torch.zeros(1, 3, 2000), torch.zeros(1, 2000, 32), torch.zeros(1, 1025, dtype=torch.long),
                          torch.zeros(1, dtype=torch.long), torch.eye(3, dtype=torch.float64)[None])
    with pytest.raises(ValueError, match="nope"):
        ops.src_keypoints(torch.zeros(1, 3, 2000), torch.zeros(1, 2000, 32), torch.zeros(1, 64, dtype=torch.long),
                          torch.zeros(1, dtype=torch.long), torch.eye(3, dtype=torch.float64)[None], method="nope")
