"""CPU-side checks of paper mode's extractor training (dvcp_feature_propagation_backward,
dvcp_group_rows_backward, DeepVCPPaper(train_extractor=True)): the ctypes prototypes against the
header, the workspace size queries against their formula, the argument checks that come back before
any launch, the opt-in flag's state_dict and the guard that stays with train_heads=True alone."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "dvcp.h")
ENTRIES = ("dvcp_feature_propagation_backward", "dvcp_group_rows_backward")
P8 = ctypes.c_void_p(16)


def _align(x):
    return (x + 255) // 256 * 256


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def _nparams(ch):
    return sum(a * b + 3 * b for a, b in zip(ch[:-1], ch[1:]))


def test_ctypes_arity_matches_header():
    from dvcp import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = dict(re.findall(r"(?:int|int64_t)\s+(dvcp_\w+)\s*\(([^)]*)\)\s*;", text))
    for name in ENTRIES:
        assert protos[name].count(",") + 1 == len(_lib.SIGNATURES[name]), name
        assert name + "_workspace_bytes" in protos and name + "_workspace_bytes" in _lib.exported_symbols()
    assert protos["dvcp_feature_propagation_backward_workspace_bytes"].count(",") + 1 == 7
    assert protos["dvcp_group_rows_backward_workspace_bytes"].count(",") + 1 == 4
    assert _lib.ABI_VERSION == 5


def test_workspace_bytes():
    """Feature propagation: one partial row of the packed gradient per workgroup, min(B ceil(N1 / 32),
    256) of them; with grad_p2 wanted the E = 3 B N1 keys, the E x D2 contribution rows and segment_sum's
    own workspace for (E entries, B N2 rows).  Group rows: the E = B Q ns keys and segment_sum's own for
    (E, B N).  segment_sum's share is not exported; it is the same function of (entries, rows) in both
    queries and holds at least its sorted keys, values and the rows' bounds."""
    import dvcp
    lib = dvcp.load_library()
    fpq, grq = lib.dvcp_feature_propagation_backward_workspace_bytes, lib.dvcp_group_rows_backward_workspace_bytes
    for ch in ([128, 64, 64], [96, 32, 32], [32, 32, 32, 32, 32], [32, 16]):
        c = _ints(*ch)
        L = len(ch) - 1
        for B, N1 in ((1, 1), (2, 31), (2, 32), (2, 33), (1, 8192), (1, 8193), (4, 16384)):
            tiles = B * -(-N1 // 32)
            assert int(fpq(B, N1, 700, 64, L, c, 0)) == _align(min(tiles, 256) * _nparams(ch) * 4), (ch, B, N1)
        assert int(fpq(0, 100, 700, 64, L, c, 1)) == 0 and int(fpq(3, 0, 700, 64, L, c, 1)) == 0
    c = _ints(96, 32, 32)
    assert int(fpq(1, 10, 0, 64, 2, c, 0)) == -1 and int(fpq(1, 10, 5, 64, 5, c, 0)) == -1
    assert int(fpq(1, 10, 5, 64, 2, None, 0)) == -1 and int(grq(1, 2, 3, 0)) == -1
    # segment_sum's share, by difference: the same for the same (entries, rows) in both queries.  Up to
    # 1024 entries here: above, the radix sort's own size query asks the device for its properties and
    # fails on a host without one (dvcp_dfe_tgt_backward_workspace_bytes does the same).
    for B, N1, N2, D2 in ((2, 64, 50, 64), (1, 300, 90, 32), (3, 100, 7, 32)):
        E = 3 * B * N1
        fixed = _align(min(B * -(-N1 // 32), 256) * _nparams([96, 32, 32]) * 4)
        assert int(fpq(B, N1, N2, D2, 2, c, 0)) == fixed
        seg = int(fpq(B, N1, N2, D2, 2, c, 1)) - fixed - _align(E * 4) - _align(E * D2 * 4)
        assert seg >= 2 * _align(E * 4) + 2 * _align(B * N2 * 4), (B, N1, N2)
        # group rows with Q ns = 3 N1 entries over B N2 points: the keys and the same share
        assert int(grq(B, N1, N2, 3)) == _align(E * 4) + seg
    assert int(grq(0, 5, 100, 32)) == 0 and int(grq(2, 0, 100, 32)) == 0 and int(grq(2, 5, 0, 32)) == 0


def _fp_call(lib_call, N1=40, N2=9, B=2, D1=32, D2=64, ch=(96, 32, 32), relu=(1, 1), ws_bytes=None, want_p2=True,
             **null):
    import dvcp
    lib = dvcp.load_library()
    L = len(ch) - 1
    c, r = _ints(*ch), _ints(*relu)
    if ws_bytes is None:
        ws_bytes = max(0, int(lib.dvcp_feature_propagation_backward_workspace_bytes(B, N1, N2, D2, L, c, int(want_p2))))
    a = dict(xyz1=P8, xyz2=P8, p1=P8, p2=P8, chans_p=ctypes.cast(c, ctypes.c_void_p), relu_p=ctypes.cast(r, ctypes.c_void_p),
             params=P8, bnstat=P8, gout=P8, gp1=P8, gp2=P8 if want_p2 else None, ws=P8, gparams=P8)
    a.update(null)
    lib_call("dvcp_feature_propagation_backward", a["xyz1"], 0, 0, 0, N1, a["xyz2"], 0, 0, 0, N2, B, a["p1"], 0, 0, 0,
             D1, a["p2"], 0, 0, D2, L, a["chans_p"], a["relu_p"], a["params"], a["bnstat"], a["gout"], a["gp1"], a["gp2"],
             a["ws"], ws_bytes, a["gparams"], None)


def test_feature_propagation_backward_rejects_bad_arguments():
    """Null pointers, five layers, a 129-wide row, a 65-wide layer, N2 = 2, D2 = 48 with grad_p2 wanted, a
    short workspace: errors before any launch (the pointers here are not device memory)."""
    import dvcp
    from dvcp import _lib
    lib = dvcp.load_library()
    name = "dvcp_feature_propagation_backward"
    for arg in ("xyz1", "xyz2", "p1", "p2", "chans_p", "relu_p", "params", "bnstat", "gout", "ws", "gparams"):
        with pytest.raises(RuntimeError, match=name + ": null pointer"):
            _fp_call(_lib.call, **{arg: None})
    with pytest.raises(RuntimeError, match=name + r": 1\.\.4 layers"):
        _fp_call(_lib.call, ch=(96, 32, 32, 32, 32, 32), relu=(1, 1, 1, 1, 1), ws_bytes=1 << 20)
    with pytest.raises(RuntimeError, match=name + ": layer width 129 out of range"):
        _fp_call(_lib.call, D1=65, ch=(129, 32, 32))
    with pytest.raises(RuntimeError, match=name + ": layer width 65 out of range"):
        _fp_call(_lib.call, ch=(96, 65, 32))
    with pytest.raises(RuntimeError, match=name + ": N2 = 2"):
        _fp_call(_lib.call, N2=2)
    with pytest.raises(RuntimeError, match=name + r": chans\[0\]=96 != D1 \+ D2"):
        _fp_call(_lib.call, D1=0)
    with pytest.raises(RuntimeError, match=name + r": grad_p2 with D2=48 \(segment_sum takes 32 or 64 columns\)"):
        _fp_call(_lib.call, D1=48, D2=48, ws_bytes=1 << 24)
    c = _ints(96, 32, 32)
    for want_p2 in (False, True):
        need = int(lib.dvcp_feature_propagation_backward_workspace_bytes(2, 40, 9, 64, 2, c, int(want_p2)))
        assert need > 0
        with pytest.raises(RuntimeError, match=rf"workspace of {need - 4} bytes is short of {need}"):
            _fp_call(_lib.call, ws_bytes=need - 4, want_p2=want_p2)
    with pytest.raises(RuntimeError, match="workspace of 0 bytes is short"):
        _fp_call(_lib.call, ws_bytes=0)
    # no row: the parameter pointers are still needed
    with pytest.raises(RuntimeError, match=name + ": null pointer"):
        _fp_call(_lib.call, N1=0, gparams=None)


def test_group_rows_backward_rejects_bad_arguments():
    import dvcp
    from dvcp import _lib
    lib = dvcp.load_library()
    name = "dvcp_group_rows_backward"
    need = int(lib.dvcp_group_rows_backward_workspace_bytes(2, 5, 100, 32))
    assert need > 0

    def call(D=32, count=P8, lst=P8, g=P8, gf=P8, ws=P8, ws_bytes=need, ns_list=20):
        _lib.call(name, count, lst, ns_list, 32, 5, 100, D, 2, g, gf, ws, ws_bytes, None)

    for D in (16, 0, 64):
        with pytest.raises(RuntimeError, match=name + rf": D={D} \(32 feature columns only\)"):
            call(D=D)
    for arg in ("count", "lst", "g", "gf", "ws"):
        with pytest.raises(RuntimeError, match=name + ": null pointer"):
            call(**{arg: None})
    with pytest.raises(RuntimeError, match=name + ": bad sizes"):
        call(ns_list=0)
    with pytest.raises(RuntimeError, match=rf"workspace of {need - 4} bytes is short of {need}"):
        call(ws_bytes=need - 4)


def test_train_extractor_leaves_state_dict_alone():
    import dvcp
    cfg = dict(use_normal=False, npoints=(16, 8, 4))
    a, b = dvcp.paper.DeepVCPPaper(**cfg), dvcp.paper.DeepVCPPaper(train_extractor=True, **cfg)
    assert not a.train_extractor and b.train_extractor and not b.train_heads
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())
    assert not any("train_extractor" in k for k in b.state_dict())
    a.load_state_dict(b.state_dict())


def test_guards_without_a_gpu():
    """train_heads=True alone goes on refusing a trainable extractor with its present message;
    train_extractor=True lets it through to the operands (CPU tensors here); .train() stays refused."""
    import dvcp
    args = (torch.rand(1, 3, 64), torch.rand(1, 3, 64), torch.eye(3, dtype=torch.float64)[None], torch.zeros(1, 3))
    m = dvcp.paper.DeepVCPPaper(use_normal=False, train_heads=True, npoints=(16, 8, 4)).eval()
    with pytest.raises(NotImplementedError, match=r"extractor must be frozen \(model.FE.requires_grad_\(False\)\)"):
        m(*args)
    m.train_extractor = True
    with pytest.raises(RuntimeError, match="no GPU|expected a GPU tensor"):
        m(*args)
    with pytest.raises(NotImplementedError, match="training mode"):
        m.train()(*args)
    # the modules on their own: eval mode with a trainable parameter takes the autograd path (no CPU fallback)
    fe = dvcp.paper.PaperFeatExtraction(npoints=(16, 8, 4)).eval()
    with pytest.raises(RuntimeError, match="no GPU|expected a GPU tensor"):
        fe(torch.rand(1, 3, 64))
    with pytest.raises(NotImplementedError, match="training mode"):
        fe.train()(torch.rand(1, 3, 64))
    # a grid above 11^3 is refused when it would be recorded, as with train_heads
    big = dvcp.paper.DeepVCPPaper(use_normal=False, train_extractor=True, r=2.4, s=0.4, npoints=(16, 8, 4)).eval()
    with pytest.raises(NotImplementedError, match="inference-only"):
        big(*args)
