"""CPU-side checks of paper mode's batch-statistics BatchNorm (dvcp_weighting_bn_stats / _forward /
_backward, the paper's sa1 tables in dvcp_sa_bn_*, ``bn_train``): the ctypes prototypes against the
header, the workspace size queries, the argument checks that come back before any launch, the opt-in
flag's state_dict and its way to the children, and the refusals that fire before the operands are
looked at."""
import os
import re

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "dvcp.h")
WL_NPARAMS = 32 * 16 + 16 + 16 * 8 + 8 + 8 + 1
WL_BN_NPARAMS = WL_NPARAMS + 2 * (16 + 8)
ENTRIES = ("dvcp_weighting_bn_stats", "dvcp_weighting_bn_forward", "dvcp_weighting_bn_backward")


def test_ctypes_arity_matches_header():
    from dvcp import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = dict(re.findall(r"(?:int|int64_t)\s+(dvcp_\w+)\s*\(([^)]*)\)\s*;", text))
    for name in ENTRIES:
        assert protos[name].count(",") + 1 == len(_lib.SIGNATURES[name]), name
    for name in ENTRIES:
        assert protos[name + "_workspace_bytes"].strip() == "int P"
        assert name + "_workspace_bytes" in _lib.exported_symbols()
    assert protos["dvcp_weighting_bn_nparams"].strip() == "void"
    assert _lib.ABI_VERSION == 5


def test_workspace_bytes_and_pack_size():
    """One partial row per workgroup, min(ceil(P / 64), 256) workgroups (64-row tiles): 32 doubles for
    the statistics, the 673 gradient floats for the backward (its sums' 32 doubles fit inside);
    nothing for P <= 0."""
    import dvcp
    from dvcp import ops
    lib = dvcp.load_library()
    assert int(lib.dvcp_weighting_bn_nparams()) == WL_BN_NPARAMS == 721 == ops.WEIGHTING_BN_NPARAMS
    assert ops.WEIGHTING_BN_NSTAT == 96 and WL_NPARAMS * 4 >= 32 * 8
    for P in (0, -1, -100):
        assert int(lib.dvcp_weighting_bn_stats_workspace_bytes(P)) == 0
        assert int(lib.dvcp_weighting_bn_backward_workspace_bytes(P)) == 0
        assert int(lib.dvcp_weighting_bn_forward_workspace_bytes(P)) == 0
    for P in (1, 2, 63, 64, 65, 1000, 16384, 16385, 16449, 1 << 20):
        grid = min(-(-P // 64), 256)
        assert int(lib.dvcp_weighting_bn_stats_workspace_bytes(P)) == grid * 32 * 8, P
        assert int(lib.dvcp_weighting_bn_backward_workspace_bytes(P)) == grid * WL_NPARAMS * 4, P
        assert int(lib.dvcp_weighting_bn_forward_workspace_bytes(P)) == 0   # a row per lane, nothing shared


def test_weighting_bn_entry_points_reject_bad_arguments():
    import dvcp
    from dvcp import _lib
    lib = dvcp.load_library()
    P8 = _lib.ctypes.c_void_p(16)
    need_s = int(lib.dvcp_weighting_bn_stats_workspace_bytes(100))
    need_b = int(lib.dvcp_weighting_bn_backward_workspace_bytes(100))

    def stats(P=100, feat=P8, params=P8, layer=1, ws=P8, ws_bytes=need_s, sums=P8):
        _lib.call("dvcp_weighting_bn_stats", feat, P, params, layer, ws, ws_bytes, sums, None)

    with pytest.raises(RuntimeError, match="dvcp_weighting_bn_stats: P=-2 is negative"):
        stats(P=-2)
    for layer in (0, 3, -1):
        with pytest.raises(RuntimeError, match=rf"dvcp_weighting_bn_stats: layer {layer} out of range \(1, 2\)"):
            stats(layer=layer)
    for arg in ("feat", "params", "ws", "sums"):
        with pytest.raises(RuntimeError, match="dvcp_weighting_bn_stats: null pointer"):
            stats(**{arg: None})
    with pytest.raises(RuntimeError, match="dvcp_weighting_bn_stats: null pointer"):
        stats(P=0, sums=None)
    with pytest.raises(RuntimeError, match=rf"workspace of {need_s - 8} bytes is short of {need_s}"):
        stats(ws_bytes=need_s - 8)

    def forward(P=100, feat=P8, params=P8, score=P8):
        _lib.call("dvcp_weighting_bn_forward", feat, P, params, score, None)

    with pytest.raises(RuntimeError, match="dvcp_weighting_bn_forward: P=-1 is negative"):
        forward(P=-1)
    for arg in ("feat", "params", "score"):
        with pytest.raises(RuntimeError, match="dvcp_weighting_bn_forward: null pointer"):
            forward(**{arg: None})
    forward(P=0, feat=None, score=None)   # no row: nothing to read or write

    def backward(P=100, feat=P8, params=P8, stat=P8, gs=P8, mode=0, ws=P8, ws_bytes=need_b, sums=P8, gp=P8):
        _lib.call("dvcp_weighting_bn_backward", feat, P, params, stat, gs, mode, P8, ws, ws_bytes, sums, gp, None)

    with pytest.raises(RuntimeError, match="dvcp_weighting_bn_backward: P=-2 is negative"):
        backward(P=-2)
    for mode in (-1, 3):
        with pytest.raises(RuntimeError, match=rf"dvcp_weighting_bn_backward: mode {mode} out of range \(0\.\.2\)"):
            backward(mode=mode)
    for arg in ("feat", "params", "stat", "gs", "ws", "gp"):
        with pytest.raises(RuntimeError, match="dvcp_weighting_bn_backward: null pointer"):
            backward(**{arg: None})
    for mode in (1, 2):   # the output of the mode is the one that must be there
        with pytest.raises(RuntimeError, match="dvcp_weighting_bn_backward: null pointer"):
            backward(mode=mode, sums=None)
        with pytest.raises(RuntimeError, match="workspace of 0 bytes is short"):
            backward(mode=mode, gp=None, ws_bytes=0)
    with pytest.raises(RuntimeError, match="dvcp_weighting_bn_backward: null pointer"):
        backward(P=0, gp=None)
    with pytest.raises(RuntimeError, match=rf"workspace of {need_b - 4} bytes is short of {need_b}"):
        backward(ws_bytes=need_b - 4)


def test_paper_sa1_tables_are_known_to_the_bn_passes():
    """dvcp_sa_bn_supported answers from the list dvcp_sa_bn_stats / _zrows / _backward dispatch on
    (DVCP_BN_TABLES): the paper's sa1 (3[+3] -> 32, 32) is in it beside the four reference tables, and
    a table that is in no list is still named as unsupported by the entry point itself (with one
    centre, which reaches the lookup, before any launch)."""
    import dvcp
    from dvcp import _lib
    lib = dvcp.load_library()
    P8 = _lib.ctypes.c_void_p(16)

    def known(chans):
        ch = torch.tensor(chans, dtype=torch.int32)
        return int(lib.dvcp_sa_bn_supported(len(chans) - 1, ch.data_ptr()))

    for chans in ((3, 16, 16, 32), (6, 16, 16, 32), (35, 32, 64), (67, 64, 64), (3, 32, 32), (6, 32, 32)):
        assert known(chans) == 1, chans
    for chans in ((3, 32, 48), (4, 32, 32), (35, 32, 32), (3, 32, 32, 32), (3, 32)):
        assert known(chans) == 0, chans
    assert int(lib.dvcp_sa_bn_supported(2, None)) == 0
    for chans in ((3, 32, 32), (6, 32, 32)):
        ch = torch.tensor(chans, dtype=torch.int32)
        assert int(lib.dvcp_sa_bn_pack_floats(2, ch.data_ptr())) == sum(a * b + 7 * b for a, b in zip(chans, chans[1:]))
        assert int(lib.dvcp_sa_bn_zrows_floats(1, 3, 32, 2, ch.data_ptr())) == 64 * 128
        assert int(lib.dvcp_sa_bn_workspace_bytes(1, 3, 2, ch.data_ptr())) > 0
        assert not lib.dvcp_sa_bnm_supported(2, ch.data_ptr())   # the matrix-core path does not take it
    ch = torch.tensor((3, 32, 48), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="dvcp_sa_bn_zrows: unsupported table D=0 chans=32,48"):
        _lib.call("dvcp_sa_bn_zrows", _lib.F32, P8, 0, 0, 0, 8, P8, 0, 0, 0, 1, 1, _lib.F32, None, 0, 0, 0, 0, P8, P8, 4,
                  2, ch.data_ptr(), P8, P8, None)


def test_bn_train_leaves_state_dict_alone_and_reaches_the_heads():
    import dvcp
    cfg = dict(use_normal=False, npoints=(16, 8, 4))
    a, b = dvcp.paper.DeepVCPPaper(**cfg), dvcp.paper.DeepVCPPaper(bn_train=True, **cfg)
    assert not a.bn_train and b.bn_train
    assert list(a.state_dict()) == list(b.state_dict())
    assert not any("bn_train" in k for k in b.state_dict())
    a.load_state_dict(b.state_dict())
    assert all(st.WL.bn_train for st in b.stages) and not any(st.WL.bn_train for st in a.stages)
    assert b.FE.bn_train and all(fp.bn_train for fp in (b.FE.fp1, b.FE.fp2, b.FE.fp3))
    assert not a.FE.bn_train and not any(fp.bn_train for fp in (a.FE.fp1, a.FE.fp2, a.FE.fp3))
    fa, fb = dvcp.paper.PaperFeatExtraction(npoints=(16, 8, 4)), dvcp.paper.PaperFeatExtraction(bn_train=True, npoints=(16, 8, 4))
    assert list(fa.state_dict()) == list(fb.state_dict()) and all(fp.bn_train for fp in (fb.fp1, fb.fp2, fb.fp3))
    pa, pb = dvcp.paper.PointNetFeaturePropagation(35, [32, 32]), dvcp.paper.PointNetFeaturePropagation(35, [32, 32], bn_train=True)
    assert not pa.bn_train and pb.bn_train and list(pa.state_dict()) == list(pb.state_dict())
    wa, wb = dvcp.paper.PaperWeighting(), dvcp.paper.PaperWeighting(bn_train=True)
    assert not wa.bn_train and wb.bn_train and list(wa.state_dict()) == list(wb.state_dict())
    assert [n for n, _ in wa.named_parameters()] == [n for n, _ in wb.named_parameters()]


def test_refusals_come_before_the_operands():
    """Without the flag .train() is refused with the message it always had; with it, a single row
    raises torch's ValueError and an extractor in training mode the flag's own refusal -- all on CPU
    tensors, so before the "no GPU" error."""
    import dvcp
    wl = dvcp.paper.PaperWeighting().train()
    with pytest.raises(NotImplementedError, match="PaperWeighting.forward in training mode"):
        wl(torch.zeros(1, 4, 32))
    wl = dvcp.paper.PaperWeighting(bn_train=True).train()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        wl(torch.zeros(1, 1, 32))
    with pytest.raises(RuntimeError, match="no GPU|expected a GPU tensor"):
        wl(torch.zeros(1, 4, 32))
    with pytest.raises(RuntimeError, match="no GPU|expected a GPU tensor"):   # eval mode: the eval path
        wl.eval()(torch.zeros(1, 1, 32))
    cfg = dict(use_normal=False, npoints=(16, 8, 4))
    args = (torch.rand(1, 3, 64), torch.rand(1, 3, 64), torch.eye(3, dtype=torch.float64)[None], torch.zeros(1, 3))
    m = dvcp.paper.DeepVCPPaper(**cfg).train()
    with pytest.raises(NotImplementedError, match="DeepVCPPaper.forward in training mode"):
        m(*args)
    m = dvcp.paper.DeepVCPPaper(bn_train=True, **cfg).train()   # the whole network in train mode goes on to its operands
    with pytest.raises(RuntimeError, match="no GPU|expected a GPU tensor"):
        m(*args)
    m.FE.eval()
    with pytest.raises(RuntimeError, match="no GPU|expected a GPU tensor"):
        m(*args)
    # the propagation: one row raises torch's ValueError before the "no GPU" error
    fp = dvcp.paper.PointNetFeaturePropagation(35, [32, 32], bn_train=True).train()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        fp(torch.zeros(1, 3, 1), torch.zeros(1, 3, 4), torch.zeros(1, 3, 1), torch.zeros(1, 32, 4))
    with pytest.raises(RuntimeError, match="no GPU|expected a GPU tensor"):
        fp(torch.zeros(1, 3, 2), torch.zeros(1, 3, 4), torch.zeros(1, 3, 2), torch.zeros(1, 32, 4))
    fe = dvcp.paper.PaperFeatExtraction(bn_train=True, npoints=(16, 8, 4)).train()
    with pytest.raises(RuntimeError, match="no GPU|expected a GPU tensor"):
        fe(torch.rand(1, 3, 64))
    # built without the flag, all four classes with BatchNorm refuse .train() as they always did; so does
    # CPG1D, which has no BatchNorm and no flag
    P = dvcp.paper
    x = torch.zeros(1, 3, 8)
    for mod, a in ((P.PointNetFeaturePropagation(35, [32, 32]), (x, x, torch.zeros(1, 3, 8), torch.zeros(1, 32, 8))),
                   (P.PaperFeatExtraction(npoints=(16, 8, 4)), (torch.rand(1, 3, 64),)),
                   (P.PaperWeighting(), (torch.zeros(1, 4, 32),)), (P.DeepVCPPaper(**cfg), args),
                   (P.CPG1D(), [torch.zeros(1, 1, 32)] * 3)):
        with pytest.raises(NotImplementedError, match=f"{type(mod).__name__}.forward in training mode"):
            mod.train()(*a)


FP_ENTRIES = ("dvcp_feature_propagation_bn_stats", "dvcp_feature_propagation_bn_backward")


def test_feature_propagation_bn_entry_points():
    """Arity against the header, the workspace formulas (one partial row of 128 doubles per workgroup and
    row quarter, min(tiles, 256) workgroups, added to the eval backward's workspace) and every argument
    refusal, before any launch."""
    import dvcp
    from dvcp import _lib
    lib = dvcp.load_library()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = dict(re.findall(r"(?:int|int64_t)\s+(dvcp_\w+)\s*\(([^)]*)\)\s*;", text))
    for name in FP_ENTRIES:
        assert protos[name].count(",") + 1 == len(_lib.SIGNATURES[name]), name
        assert name + "_workspace_bytes" in protos and name + "_workspace_bytes" in _lib.exported_symbols()
    ch = torch.tensor([96, 32, 32], dtype=torch.int32)
    for B, N1 in ((0, 5), (2, 0)):
        assert int(lib.dvcp_feature_propagation_bn_stats_workspace_bytes(B, N1)) == 0
        assert int(lib.dvcp_feature_propagation_bn_backward_workspace_bytes(B, N1, 9, 64, 2, ch.data_ptr(), 1)) == 0
    assert int(lib.dvcp_feature_propagation_bn_stats_workspace_bytes(-1, 5)) == -1
    for B, N1 in ((1, 1), (2, 33), (1, 8193), (4, 16384)):
        sums = min(B * -(-N1 // 32), 256) * 4 * 128 * 8
        assert int(lib.dvcp_feature_propagation_bn_stats_workspace_bytes(B, N1)) == sums, (B, N1)
        for want_p2 in (0, 1):
            base = int(lib.dvcp_feature_propagation_backward_workspace_bytes(B, N1, 9, 64, 2, ch.data_ptr(), want_p2))
            mine = int(lib.dvcp_feature_propagation_bn_backward_workspace_bytes(B, N1, 9, 64, 2, ch.data_ptr(), want_p2))
            assert mine == (base + sums if base >= 0 else base)   # (the segment sum's size query may need a device)
    P8 = _lib.ctypes.c_void_p(16)
    rl = torch.tensor([1, 1], dtype=torch.int32)
    need_s = int(lib.dvcp_feature_propagation_bn_stats_workspace_bytes(2, 33))
    need_b = int(lib.dvcp_feature_propagation_bn_backward_workspace_bytes(2, 33, 9, 64, 2, ch.data_ptr(), 0))

    def operands(N1=33, N2=9, B=2, D1=32, D2=64, nlayer=2, chans=ch.data_ptr(), relu=rl.data_ptr(), x1=P8, p2=P8):
        return (x1, 0, 0, 0, N1, P8, 0, 0, 0, N2, B, P8, 0, 0, 0, D1, p2, 0, 0, D2, nlayer, chans, relu)

    def stats(layer=1, params=P8, ws=P8, ws_bytes=need_s, sums=P8, **kw):
        _lib.call("dvcp_feature_propagation_bn_stats", *operands(**kw), params, layer, ws, ws_bytes, sums, None)

    def backward(mode=0, params=P8, stat=P8, g=P8, ws=P8, ws_bytes=need_b, sums=P8, gp=P8, gp2=None, **kw):
        _lib.call("dvcp_feature_propagation_bn_backward", *operands(**kw), params, stat, g, mode, None, gp2, ws, ws_bytes,
                  sums, gp, None)

    for fn, who in ((stats, FP_ENTRIES[0]), (backward, FP_ENTRIES[1])):
        with pytest.raises(RuntimeError, match=f"{who}: N2 = 2"):
            fn(N2=2)
        with pytest.raises(RuntimeError, match=f"{who}: bad sizes"):
            fn(N2=0)
        with pytest.raises(RuntimeError, match=f"{who}: 1..4 layers"):
            fn(nlayer=5)
        with pytest.raises(RuntimeError, match=rf"{who}: chans\[0\]=96 != D1 \+ D2"):
            fn(D1=3)
        for arg in ("chans", "relu", "params", "x1", "p2", "ws"):
            with pytest.raises(RuntimeError, match=f"{who}: null pointer"):
                fn(**{arg: None})
    for layer in (0, 3):
        with pytest.raises(RuntimeError, match=f"layer {layer} of 2"):
            stats(layer=layer)
    with pytest.raises(RuntimeError, match="null pointer"):
        stats(sums=None)
    with pytest.raises(RuntimeError, match=rf"workspace of {need_s - 8} bytes is short of {need_s}"):
        stats(ws_bytes=need_s - 8)
    for mode in (-1, 3):
        with pytest.raises(RuntimeError, match=f"mode {mode} of 2"):
            backward(mode=mode)
    for arg, mode in (("stat", 0), ("g", 0), ("gp", 0), ("sums", 1), ("sums", 2)):
        with pytest.raises(RuntimeError, match="null pointer"):
            backward(mode=mode, **{arg: None})
    with pytest.raises(RuntimeError, match=rf"workspace of {need_b - 4} bytes is short of {need_b}"):
        backward(ws_bytes=need_b - 4)
    wide = torch.tensor([51, 32, 32], dtype=torch.int32)
    with pytest.raises(RuntimeError, match=r"grad_p2 with D2=48"):
        backward(D1=3, D2=48, chans=wide.data_ptr(), gp2=P8)
