"""CPU-side checks of paper mode's head training (dvcp_cpg1d_backward, dvcp_weighting_backward,
DeepVCPPaper(train_heads=True)): the ctypes prototypes against the header, the workspace size
queries, the argument checks that come back before any launch, the opt-in flag's state_dict and the
frozen-extractor guard."""
import os
import re

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "dvcp.h")
CPG1D_NPARAMS = 16 * 32 * 3 + 16 + 4 * 16 * 3 + 4 + 4 * 3 + 1
WL_NPARAMS = 32 * 16 + 16 + 16 * 8 + 8 + 8 + 1
ENTRIES = ("dvcp_cpg1d_backward", "dvcp_weighting_backward")


def test_ctypes_arity_matches_header():
    from dvcp import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = dict(re.findall(r"(?:int|int64_t)\s+(dvcp_\w+)\s*\(([^)]*)\)\s*;", text))
    for name in ENTRIES:
        assert protos[name].count(",") + 1 == len(_lib.SIGNATURES[name]), name
        assert name + "_workspace_bytes" in protos and name + "_workspace_bytes" in _lib.exported_symbols()
        assert protos[name + "_workspace_bytes"].strip() == "int P"
    assert _lib.ABI_VERSION == 5


def test_workspace_bytes():
    """One partial row of packed parameter gradients per workgroup: min(P, 256) workgroups for the
    1-D CPG (one key point each, then strided), min(ceil(P / 64), 256) for the weighting layer (64-row
    tiles); nothing for P <= 0."""
    import dvcp
    lib = dvcp.load_library()
    assert CPG1D_NPARAMS == 1761 == int(lib.dvcp_cpg1d_nparams()) and WL_NPARAMS == 673
    for P in (0, -1, -100):
        assert int(lib.dvcp_cpg1d_backward_workspace_bytes(P)) == 0
        assert int(lib.dvcp_weighting_backward_workspace_bytes(P)) == 0
    for P in (1, 2, 63, 64, 65, 255, 256, 257, 1000, 16384, 16385, 1 << 20):
        assert int(lib.dvcp_cpg1d_backward_workspace_bytes(P)) == min(P, 256) * CPG1D_NPARAMS * 4, P
        assert int(lib.dvcp_weighting_backward_workspace_bytes(P)) == min(-(-P // 64), 256) * WL_NPARAMS * 4, P


def test_cpg1d_backward_rejects_bad_arguments():
    """Gz out of range, null pointers, a short workspace: errors before any launch."""
    import dvcp
    from dvcp import _lib
    lib = dvcp.load_library()
    P8 = _lib.ctypes.c_void_p(16)
    need = int(lib.dvcp_cpg1d_backward_workspace_bytes(3))

    def call(P=3, Gz=9, src=P8, tgt=P8, cand=P8, params=P8, gv=P8, ws=P8, ws_bytes=need, gp=P8):
        _lib.call("dvcp_cpg1d_backward", src, tgt, cand, P, Gz, params, gv, P8, P8, ws, ws_bytes, gp, None)

    for Gz in (0, 65, -1):
        with pytest.raises(RuntimeError, match=rf"dvcp_cpg1d_backward: Gz={Gz} unsupported \(1\.\.64\)"):
            call(Gz=Gz)
    with pytest.raises(RuntimeError, match="dvcp_cpg1d_backward: Gz=9 unsupported .*P=-1"):
        call(P=-1)
    for arg in ("src", "tgt", "cand", "params", "gv", "ws", "gp"):
        with pytest.raises(RuntimeError, match="dvcp_cpg1d_backward: null pointer"):
            call(**{arg: None})
    for P in (0, 3):   # the parameter pointers are needed even with no key point
        with pytest.raises(RuntimeError, match="dvcp_cpg1d_backward: null pointer"):
            call(P=P, gp=None)
    with pytest.raises(RuntimeError, match=rf"workspace of {need - 4} bytes is short of {need}"):
        call(ws_bytes=need - 4)
    with pytest.raises(RuntimeError, match="workspace of 0 bytes is short"):
        call(ws_bytes=0)


def test_weighting_backward_rejects_bad_arguments():
    import dvcp
    from dvcp import _lib
    lib = dvcp.load_library()
    P8 = _lib.ctypes.c_void_p(16)
    need = int(lib.dvcp_weighting_backward_workspace_bytes(100))
    assert need == 2 * WL_NPARAMS * 4

    def call(P=100, feat=P8, params=P8, gs=P8, ws=P8, ws_bytes=need, gp=P8):
        _lib.call("dvcp_weighting_backward", feat, P, params, gs, P8, ws, ws_bytes, gp, None)

    with pytest.raises(RuntimeError, match="dvcp_weighting_backward: P=-2 is negative"):
        call(P=-2)
    for arg in ("feat", "params", "gs", "ws", "gp"):
        with pytest.raises(RuntimeError, match="dvcp_weighting_backward: null pointer"):
            call(**{arg: None})
    with pytest.raises(RuntimeError, match="dvcp_weighting_backward: null pointer"):
        call(P=0, params=None)
    with pytest.raises(RuntimeError, match=rf"workspace of {need - 4} bytes is short of {need}"):
        call(ws_bytes=need - 4)


def test_train_heads_leaves_state_dict_alone():
    import dvcp
    cfg = dict(use_normal=False, npoints=(16, 8, 4))
    a, b = dvcp.paper.DeepVCPPaper(**cfg), dvcp.paper.DeepVCPPaper(train_heads=True, **cfg)
    assert not a.train_heads and b.train_heads
    assert list(a.state_dict()) == list(b.state_dict())
    assert not any("train_heads" in k for k in b.state_dict())
    a.load_state_dict(b.state_dict())


def test_frozen_extractor_guard_comes_first():
    """DeepVCPPaper(train_heads=True) with a trainable extractor parameter is refused before the
    operands are looked at: with or without a GPU the error is the guard's, not "no GPU"."""
    import dvcp
    m = dvcp.paper.DeepVCPPaper(use_normal=False, train_heads=True, npoints=(16, 8, 4)).eval()
    args = (torch.rand(1, 3, 64), torch.rand(1, 3, 64), torch.eye(3, dtype=torch.float64)[None], torch.zeros(1, 3))
    with pytest.raises(NotImplementedError, match=r"extractor must be frozen \(model.FE.requires_grad_\(False\)\)"):
        m(*args)
    m.FE.requires_grad_(False)
    m.FE.sa2.mlp_bns[0].bias.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="extractor must be frozen"):
        m(*args)
    with pytest.raises(NotImplementedError, match="training mode"):
        m.train()(*args)
    # frozen: the forward goes on to its operands, which are CPU tensors here
    m.eval().FE.requires_grad_(False)
    with pytest.raises(RuntimeError, match="no GPU|expected a GPU tensor"):
        m(*args)
    # a grid above 11^3 is refused when it would be recorded, as in dvcp.DeepVCP
    big = dvcp.paper.DeepVCPPaper(use_normal=False, train_heads=True, r=2.4, s=0.4, npoints=(16, 8, 4)).eval()
    big.FE.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="inference-only"):
        big(*args)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no GPU|expected a GPU tensor"):
        big(*args)
