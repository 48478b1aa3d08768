"""Every HIP entry point under poisoned allocations with guard bands (tests/memcheck.py).

The wrappers in dvcp/ops.py allocate outputs and workspaces with ``torch.empty`` and trust the
kernels to write every byte they return, to read no workspace byte before writing it, and to write
nothing outside those buffers.  The caching allocator hides a break of the first two (the block of
the previous same-shape call comes back, still holding the last correct answer) and nothing in the
suite sees the third.  Here each case (one ``ops`` call, or a forward with the backward that reads
its workspace or state) builds seeded inputs outside the hook and then runs four times: plain,
plain again, with every GPU allocation filled with 0xFF and with 0x5A.  Asserted:

* the two plain runs return the same bytes (compared through an integer view: NaN payloads and the
  sign of zero count), and so do the poisoned runs and the plain one;
* ``check()`` is empty after each poisoned run: the 512 bytes before and after every allocation
  still hold the poison byte.

Not bit-reproducible (NOT_BIT_REPRODUCIBLE below; their two plain runs differ, measured on an MI355X):
``sa_group_mlp_backward[sa2]`` / ``[sa3]`` (output 1, the feature gradient: csrc/sa_bwd.hip adds each
entry's row with a float atomicAdd; the plain runs differed by 1.2e-7 and 6.0e-8 of a 1.3 / 1.2 maximum),
``src_keypoints_backward[K=64,*]`` (output 0, csrc/keypoints.hip's atomicAdd; 3.6e-7 of 1.5) and
``src_keypoints_backward_ws[K=257,*]`` (output 3, csrc/keypoints_split.hip's; 4.2e-7 of 1.2).  For that one
output the poisoned runs are compared with the plain run under the bound its parity test applies against
the oracle (max |a - b| <= 1e-4 resp. 1e-5 of max |b|); their other outputs, every other case and the three
composite passes are bit-identical.

Unspecified output regions (UNSPECIFIED below, masked by an output of the same call):
* ``ops.ball_query``'s compact ``list`` beyond ``count[b, s]``: include/dvcp.h, dvcp_ball_query:
  "list B x S x nsample int32 (the hits, ascending; entries >= count undefined)"; entry 0 of a centre
  without hits is specified (point 0, tests/test_gpu_kernels.py::test_ball_query_no_hit_compact_row)
  and is compared.

The coverage gate at the end logs the entry points the cases reach through ``_lib.call`` and
``ops.call`` and fails for any exported symbol that no case reached and EXCLUDED does not name.
"""
import contextlib
import functools

import pytest
import torch

from memcheck import POISONS, Poison, bits

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------
# the case table: name -> builder(cuda) -> run() -> tuple of outputs

CASES = {}
SEEN = set()      # entry points reached while cases ran
_RAN = set()      # cases that ran (under the logger)


def case(name):
    def deco(fn):
        assert name not in CASES, name
        CASES[name] = fn
        return fn
    return deco


# case -> (index of the one output that may differ, relative tolerance of max |a - b| against max |b|, the
# parity test the tolerance is taken from).  Every other output of the case is held to bit identity.
# Reason, all six: a float atomicAdd in the feature scatter; the order of a row's additions is not fixed.
NOT_BIT_REPRODUCIBLE = {
    "sa_group_mlp_backward[sa2]": (1, 1e-4, "test_gpu_train.py::test_sa_backward_vs_oracle (feature gradient)"),
    "sa_group_mlp_backward[sa3]": (1, 1e-4, "test_gpu_train.py::test_sa_backward_vs_oracle (feature gradient)"),
    "src_keypoints_backward[K=64,f32]": (0, 1e-5, "test_gpu_train.py::test_src_keypoints_feature_grad_vs_oracle"),
    "src_keypoints_backward[K=64,f64]": (0, 1e-5, "test_gpu_train.py::test_src_keypoints_feature_grad_vs_oracle"),
    "src_keypoints_backward_ws[K=257,f32]": (3, 1e-5, "test_gpu_train.py::test_src_keypoints_feature_grad_vs_oracle"),
    "src_keypoints_backward_ws[K=257,f64]": (3, 1e-5, "test_gpu_train.py::test_src_keypoints_feature_grad_vs_oracle"),
}


def _mask_ball_list(outs):
    """(count, list, padded): list entries at or beyond count are undefined (include/dvcp.h); entry 0 of a
    centre without hits is specified."""
    count, lst, pad = outs
    if lst is None:
        return outs
    col = torch.arange(lst.shape[2], device=lst.device)
    keep = col[None, None, :] < count.clamp(min=1)[..., None]
    return count, torch.where(keep, lst, torch.zeros_like(lst)), pad


UNSPECIFIED = {}   # case -> mask function; filled where the ball-query cases are defined


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _cloud(g, B, N, dtype=torch.float32, span=1.0):
    return ((torch.rand(B, N, 3, generator=g, dtype=torch.float64) * 2 - 1) * span).to(dtype)


# ---- FPS ---------------------------------------------------------------------------------------
def _fps_case(name, N, npoint, dtype, parts, B=2):
    @case(name)
    def build(cuda):
        from dvcp import ops
        g = _g(1000 + N)
        xyz = _cloud(g, B, N, dtype).to(cuda)
        start = torch.randint(0, N, (B,), generator=g).to(cuda)
        return lambda: ops.fps(xyz, npoint, start, pdim=1, parts=parts)


_fps_case("fps[register,f32,N=3000]", 3000, 750, torch.float32, None)
_fps_case("fps[register,f64,N=1500]", 1500, 375, torch.float64, None)
_fps_case("fps[small,f32,N=333]", 333, 400, torch.float32, None)           # below the select kernel; npoint > N
_fps_case("fps[workspace,f32,N=16385]", 16385, 96, torch.float32, 1)       # just above FPS_REG_LIMIT: per-step split
_fps_case("fps[workspace,f64,N=8193]", 8193, 96, torch.float64, None)
_fps_case("fps[parts=2,N=4096]", 4096, 1024, torch.float32, 2)
_fps_case("fps[parts=8,N=2048]", 2048, 512, torch.float32, 8)              # FPS_PART_RANGE[0]
_fps_case("fps[parts=8,N=16385]", 16385, 96, torch.float32, None)          # the default above 16384 points


@case("fps_pair[N=2048]")
def _(cuda):
    from dvcp import ops
    g = _g(1010)
    xyz = _cloud(g, 2, 2048).transpose(1, 2).contiguous().to(cuda)
    s2, s3 = (torch.randint(0, 2048, (2,), generator=g).to(cuda) for _ in range(2))
    return lambda: ops.fps_pair(xyz, s2, s3, pdim=2)


def _raw_fps_case(name, entry, N, npoint, dtype, B=2):
    """dvcp_fps / dvcp_fps_ws have no ops wrapper (ops.fps calls dvcp_fps_parts)."""
    @case(name)
    def build(cuda):
        from dvcp import _lib
        g = _g(1020 + N)
        xyz = _cloud(g, B, N, dtype).to(cuda)
        start = torch.randint(0, N, (B,), generator=g).to(cuda)

        def run():
            idx = torch.empty(B, npoint, dtype=torch.int64, device=cuda)
            ctr = torch.empty(B, 3, npoint, dtype=dtype, device=cuda)
            args = (_lib.dtype_code(xyz), _lib.ptr(xyz), N * 3, 1, 3, B, N, npoint, _lib.ptr(start), _lib.ptr(idx),
                    _lib.ptr(ctr))
            if entry == "dvcp_fps":
                _lib.call(entry, *args, _lib.stream())
                return idx, ctr
            ws = torch.empty(B * N, dtype=torch.float32, device=cuda)
            err = torch.zeros(1, dtype=torch.int32, device=cuda)
            _lib.call(entry, *args, _lib.ptr(ws), _lib.ptr(err), _lib.stream())
            return idx, ctr, err
        return run


_raw_fps_case("dvcp_fps[f32,N=3000]", "dvcp_fps", 3000, 750, torch.float32)
_raw_fps_case("dvcp_fps[f64,N=700]", "dvcp_fps", 700, 200, torch.float64)
_raw_fps_case("dvcp_fps_ws[f32,N=3000]", "dvcp_fps_ws", 3000, 750, torch.float32)
_raw_fps_case("dvcp_fps_ws[f32,N=16385]", "dvcp_fps_ws", 16385, 96, torch.float32)


# ---- ball query --------------------------------------------------------------------------------
def _ball_inputs(cuda, N, S, dtype, seed):
    g = _g(seed)
    xyz = _cloud(g, 2, N, dtype)
    ctr = xyz[:, :S].clone()
    ctr[:, ::3] = 50.0                      # every third centre far from every point: no hits
    return xyz.to(cuda), ctr.contiguous().to(cuda)


def _ball_case(name, N, S, dtype, ns, radius, compact, padded):
    @case(name)
    def build(cuda):
        from dvcp import ops
        xyz, ctr = _ball_inputs(cuda, N, S, dtype, 1100 + N + S)
        return lambda: ops.ball_query(xyz, ctr, radius, ns, compact=compact, padded=padded)
    UNSPECIFIED[name] = _mask_ball_list


_ball_case("ball_query[f32,both]", 3000, 257, torch.float32, 16, 0.2, True, True)
_ball_case("ball_query[f32,compact]", 3000, 257, torch.float32, 64, 0.2, True, False)
_ball_case("ball_query[f32,padded]", 3000, 257, torch.float32, 16, 0.2, False, True)
_ball_case("ball_query[f64,both]", 3000, 257, torch.float64, 16, 0.2, True, True)
_ball_case("ball_query[f64,compact]", 1000, 77, torch.float64, 64, 0.3, True, False)
_ball_case("ball_query[f32,N=20000]", 20000, 130, torch.float32, 32, 0.1, True, True)    # the large bitmap
_ball_case("ball_query[f32,N=66000]", 66000, 130, torch.float32, 32, 0.1, True, True)    # the streaming kernel


def _raw_ball_case(name, dtype):
    """dvcp_ball_query (no workspace) has no ops wrapper."""
    @case(name)
    def build(cuda):
        from dvcp import _lib
        N, S, ns = 3000, 257, 16
        xyz, ctr = _ball_inputs(cuda, N, S, dtype, 1150)

        def run():
            count = torch.empty(2, S, dtype=torch.int32, device=cuda)
            lst = torch.empty(2, S, ns, dtype=torch.int32, device=cuda)
            pad = torch.empty(2, S, ns, dtype=torch.int64, device=cuda)
            _lib.call("dvcp_ball_query", _lib.dtype_code(xyz), _lib.ptr(xyz), N * 3, 1, 3, N, _lib.ptr(ctr), S * 3, 1,
                      3, S, 2, 0.2, ns, _lib.ptr(count), _lib.ptr(lst), _lib.ptr(pad), _lib.stream())
            return count, lst, pad
        return run
    UNSPECIFIED[name] = _mask_ball_list


_raw_ball_case("dvcp_ball_query[f32]", torch.float32)
_raw_ball_case("dvcp_ball_query[f64]", torch.float64)


# ---- square_distance, voxelize, points_pack4 ---------------------------------------------------
def _sqd_case(dtype):
    @case(f"square_distance[{str(dtype)[6:]}]")
    def build(cuda):
        from dvcp import ops
        g = _g(1200)
        a, b = _cloud(g, 2, 301, dtype).to(cuda), _cloud(g, 2, 707, dtype).to(cuda)
        return lambda: (ops.square_distance(a, b),)


_sqd_case(torch.float32)
_sqd_case(torch.float64)


def _voxel_case(G, r, dtype):
    @case(f"voxelize[G={G},{str(dtype)[6:]}]")
    def build(cuda):
        from dvcp import ops
        pts = _cloud(_g(1210 + G), 2, 5, dtype).to(cuda)
        assert int(2 * r / 0.4 + 1) == G
        return lambda: ops.voxelize(pts, r, 0.4, G)


_voxel_case(6, 1.0, torch.float64)
_voxel_case(21, 4.0, torch.float32)


def _pack4_case(pdim):
    @case(f"points_pack4[pdim={pdim}]")
    def build(cuda):
        from dvcp import ops
        xyz = _cloud(_g(1220), 3, 901).to(cuda)
        if pdim == 2:
            xyz = xyz.transpose(1, 2).contiguous()
        return lambda: (ops.points_pack4(xyz, pdim),)


_pack4_case(1)
_pack4_case(2)


# ---- kNN ---------------------------------------------------------------------------------------
def _knn_case(method, M, Q, k, idx64):
    @case(f"knn[{method},M={M},k={k},idx64={int(idx64)}]")
    def build(cuda):
        import test_gpu_knn_slabs as KS
        from dvcp import ops
        ref, qry = KS._inputs(cuda, max(M, 200), Q, 2, seed=1300 + M + k)
        ref = ref[:, :M]
        return lambda: ops.knn(ref, qry, k, want_idx64=idx64, method=method)


for _method, _M in (("brute", 700), ("tiled", 5000), ("tiled_insert", 5000), ("tiled_slabs", 5000)):
    for _k in (1, 32):
        for _idx64 in (True, False):
            _knn_case(_method, _M, 130, _k, _idx64)
    _knn_case(_method, 20, 130, 32, True)           # fewer references than k: (inf, -1) slots
_knn_case("tiled", 16384, 130, 17, True)            # KNN_TILED_MAX_M
_knn_case("tiled_slabs", 16400, 130, 32, True)      # two slabs, a short second one
_knn_case("tiled_slabs", 16400, 130, 1, False)


# ---- set abstraction ---------------------------------------------------------------------------
def _sa_inputs(cuda, table, rows_variant):
    import test_gpu_sa_pipeline as SP
    c = SP._make(table, 3, 130, 300, None, rows_variant=rows_variant, seed=1400 + table)
    c["mine"] = c["mine"].to(cuda)
    for k in ("xyz", "ctr", "count", "lst", "feat", "rows"):
        c[k] = None if c[k] is None else c[k].to(cuda)
    assert set(c["count"].unique().tolist()) >= {0, 1, 33, c["ns"]}
    return c


def _sa_case(table, layout):
    @case(f"sa_group_mlp[sa{table + 1},{layout}]")
    def build(cuda):
        from dvcp import ops
        c = _sa_inputs(cuda, table, False)
        feat = c["feat"]
        if feat is not None:   # (B, N, D) rows -> a (B, D, N) view, point-major or channel-first memory
            feat = feat.transpose(1, 2) if layout == "point_major" else feat.transpose(1, 2).contiguous()
        sa = c["mine"]
        return lambda: (ops.sa_group_mlp(c["xyz"], c["ctr"], feat, c["count"], c["lst"], c["ns"], sa.chans,
                                         sa.packed_params(), xyz_pdim=2, feat_ddim=1, feat_pdim=2),)


for _table in (0, 1, 2):
    for _layout in ("point_major", "channel_first"):
        _sa_case(_table, _layout)


def _sa_rows_case(table):
    @case(f"sa_group_mlp_rows[sa{table + 1}]")
    def build(cuda):
        from dvcp import ops
        c = _sa_inputs(cuda, table, True)
        sa = c["mine"]
        return lambda: (ops.sa_group_mlp_rows(c["xyz"], c["ctr"], c["feat"], c["rows"], c["count"], c["lst"], c["ns"],
                                              sa.chans, sa.packed_params()),)


_sa_rows_case(1)
_sa_rows_case(2)


def _sa_plain_case(table, dtype):
    """dvcp_sa_group_mlp (no workspace) has no ops wrapper."""
    @case(f"dvcp_sa_group_mlp[sa{table + 1},{str(dtype)[6:]}]")
    def build(cuda):
        from dvcp import _lib
        c = _sa_inputs(cuda, table, False)
        sa, ns = c["mine"], c["ns"]
        xyz, ctr = c["xyz"].to(dtype), c["ctr"].to(dtype)
        feat = c["feat"].transpose(1, 2)
        B, D, N = feat.shape
        S = ctr.shape[2]
        ch = torch.tensor(list(sa.chans), dtype=torch.int32)
        params = sa.packed_params()

        def run():
            out = torch.empty(B, S, sa.chans[-1], dtype=torch.float32, device=cuda)
            st = feat.stride()
            _lib.call("dvcp_sa_group_mlp", _lib.dtype_code(xyz), _lib.ptr(xyz), xyz.stride(0), xyz.stride(1),
                      xyz.stride(2), N, _lib.ptr(ctr), ctr.stride(0), ctr.stride(1), ctr.stride(2), S, B, _lib.F32,
                      _lib.ptr(feat), st[0], st[1], st[2], D, _lib.ptr(c["count"]), _lib.ptr(c["lst"]), ns,
                      len(sa.chans) - 1, _lib.ctypes.c_void_p(ch.data_ptr()), _lib.ptr(params), _lib.ptr(out),
                      _lib.stream())
            return (out,)
        return run


_sa_plain_case(1, torch.float32)
_sa_plain_case(2, torch.float64)


# ---- head and key points -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _head_modules(cuda):
    import dvcp
    torch.manual_seed(1500)
    fe = dvcp.feat_extraction_layer(use_normal=False, npoint=16).eval().to(cuda)
    wl = dvcp.weighting_layer().eval().to(cuda)
    return fe, wl


def _fe_head_case(score):
    @case(f"fe_head[score={int(score)}]")
    def build(cuda):
        from dvcp import ops
        fe, wl = _head_modules(cuda)
        x = torch.randn(1001, 64, generator=_g(1501)).to(cuda)
        params = fe.fc_params(wl if score else None)
        return lambda: ops.fe_head(x, params, with_score=score)

    @case(f"fe_head_rows[score={int(score)}]")
    def build_rows(cuda):
        from dvcp import ops
        fe, wl = _head_modules(cuda)
        g = _g(1502)
        x = torch.randn(3, 400, 64, generator=g).to(cuda)
        rows = torch.randint(0, 400, (3, 333), generator=g).to(cuda)
        params = fe.fc_params(wl if score else None)
        return lambda: ops.fe_head_rows(x, rows, params, with_score=score)


_fe_head_case(True)
_fe_head_case(False)


@case("weighting")
def _(cuda):
    from dvcp import ops
    _, wl = _head_modules(cuda)
    feat = torch.randn(1001, 32, generator=_g(1503)).to(cuda)
    return lambda: (ops.weighting(feat, wl.packed_params()),)


def _topk_case(S, K, what):
    @case(f"topk[S={S},K={K},{what}]")
    def build(cuda):
        from dvcp import ops
        score = torch.randint(0, 4000, (3, S), generator=_g(1510 + S)).float().to(cuda) * 0.25   # with ties
        return lambda: (ops.topk(score, K),)


_topk_case(700, 64, "select1")         # csrc/head_topk.hip dvcp_topk: scores per thread 1 | 4 | 10 | 16
_topk_case(3333, 50, "select4")
_topk_case(10000, 64, "select10")
_topk_case(16384, 256, "select16")
_topk_case(3000, 1500, "argmax")       # K above kTopkMaxK = 1024: the block arg-max kernel
_topk_case(20000, 64, "stream")        # above 16384 scores: the streaming radix select


def _kp_inputs(cuda, K, dtype):
    import test_gpu_keypoints_split as KP
    xyz, feat, top, kstart = KP._float_case(K, 32, span=1.0)
    R = KP._rotations(xyz.shape[0], 7).to(cuda)
    return xyz.to(dtype).transpose(1, 2).contiguous().to(cuda), feat.to(cuda), top.to(cuda), kstart.to(cuda), R


def _kp_case(K, dtype):
    tag = "f32" if dtype == torch.float32 else "f64"

    @case(f"src_keypoints[K={K},{tag}]")
    def build(cuda):
        from dvcp import ops
        xyz, feat, top, kstart, R = _kp_inputs(cuda, K, dtype)
        return lambda: ops.src_keypoints(xyz, feat, top, kstart, R)

    if K <= 256:
        @case(f"src_keypoints_backward[K={K},{tag}]")
        def build_bwd(cuda):
            from dvcp import ops
            xyz, feat, top, kstart, R = _kp_inputs(cuda, K, dtype)
            g = torch.randn(xyz.shape[0], K, 32, 35, generator=_g(1520 + K)).to(cuda)
            return lambda: (ops.src_keypoints_backward(xyz, top, kstart, g),)
    else:
        @case(f"src_keypoints_backward_ws[K={K},{tag}]")
        def build_bwd_ws(cuda):
            from dvcp import ops
            xyz, feat, top, kstart, R = _kp_inputs(cuda, K, dtype)
            g = torch.randn(xyz.shape[0], K, 32, 35, generator=_g(1520 + K)).to(cuda)

            def run():   # the backward reads the forward's workspace
                kp, cat, moved, ws = ops.src_keypoints(xyz, feat, top, kstart, R, return_workspace=True)
                return kp, cat, moved, ops.src_keypoints_backward_ws(ws, xyz.shape[2], K, g, dtype=dtype)
            return run


for _K in (64, 257):
    for _dt in (torch.float32, torch.float64):
        _kp_case(_K, _dt)


# ---- DFE / CPG ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dfe_module(cuda):
    import dvcp
    torch.manual_seed(1600)
    return dvcp.feat_embedding_layer().eval().to(cuda)


def _dfe_case(dtype, want_input_grad):
    tag = str(dtype)[6:]

    @case(f"dfe[{tag}]")
    def build(cuda):
        from dvcp import ops
        X = torch.randn(3, 37, 32, 35, generator=_g(1601), dtype=dtype).to(cuda)      # R = 111 rows: not 64 k
        return lambda: (ops.dfe(X, _dfe_module(cuda).packed_params()),)

    @case(f"dfe_backward[{tag},input_grad={int(want_input_grad)}]")
    def build_bwd(cuda):
        from dvcp import ops
        g = _g(1602)
        X = torch.randn(3, 37, 32, 35, generator=g, dtype=dtype).to(cuda)
        go = torch.randn(3, 37, 32, generator=g).to(cuda)
        out = lambda: ops.dfe_backward(X, _dfe_module(cuda).packed_params(), go, want_input_grad=want_input_grad)
        return out if want_input_grad else (lambda: (out(),))


_dfe_case(torch.float32, True)
_dfe_case(torch.float64, False)


def _dfe_tgt_inputs(cuda, B, M, Q, seed):
    from dvcp import ops
    g = _g(seed)
    xyz = _cloud(g, B, M).transpose(1, 2).contiguous().to(cuda)                       # (B, 3, M): the FE's layout
    feat = torch.randn(B, M, 32, generator=g).to(cuda)
    qry = _cloud(g, B, Q, span=1.5).to(cuda)
    dist, idx, _ = ops.knn(xyz, qry, 32, ref_pdim=2, qry_pdim=1, want_idx64=False)
    return xyz, feat, qry, dist, idx


def _dfe_tgt_case(B, M, Q):
    for kind in ("collapsed", "literal", "f16"):
        def build(cuda, kind=kind):
            from dvcp import ops
            xyz, feat, qry, dist, idx = _dfe_tgt_inputs(cuda, B, M, Q, 1610 + Q)
            f = feat.half() if kind == "f16" else feat
            params = _dfe_module(cuda).packed_params()
            return lambda: (ops.dfe_tgt(xyz, f, qry, dist, idx, params, ref_pdim=2, literal=kind == "literal"),)
        case(f"dfe_tgt[{kind},B={B},M={M},Q={Q}]")(build)

    for feat_grad in (False, True):
        def build_bwd(cuda, feat_grad=feat_grad):
            from dvcp import ops
            xyz, feat, qry, dist, idx = _dfe_tgt_inputs(cuda, B, M, Q, 1610 + Q)
            go = torch.randn(B, Q, 32, generator=_g(1620)).to(cuda)
            params = _dfe_module(cuda).packed_params()
            out = lambda: ops.dfe_tgt_backward(xyz, feat, qry, dist, idx, params, go, ref_pdim=2,
                                               want_feat_grad=feat_grad)
            return out if feat_grad else (lambda: (out(),))
        case(f"dfe_tgt_backward[B={B},M={M},Q={Q},feat_grad={int(feat_grad)}]")(build_bwd)


_dfe_tgt_case(1, 40, 9)
_dfe_tgt_case(8, 900, 257)


@functools.lru_cache(maxsize=None)
def _cpg_module(cuda):
    import dvcp
    torch.manual_seed(1700)
    return dvcp.cpg().eval().to(cuda)


def _cpg_inputs(cuda, G, B=2, K=3):
    g = _g(1700 + G)
    C = G ** 3
    src = torch.randn(B, K, 32, generator=g).to(cuda)
    tgt = (torch.randn(B, K, C, 32, generator=g) * 0.5 + 0.3).to(cuda).permute(0, 1, 3, 2)   # the reference's view
    cand = torch.randn(B, K, C, 3, generator=g).to(cuda)
    gv = torch.randn(B, K, 3, generator=g).to(cuda)
    return src, tgt, cand, gv


def _cpg_case(G, want_weight, method=None):
    @case(f"cpg[G={G},weight={int(want_weight)}{',' + method if method else ''}]")
    def build(cuda):
        from dvcp import ops
        src, tgt, cand, _ = _cpg_inputs(cuda, G)
        params = _cpg_module(cuda).packed_params()
        out = lambda: ops.cpg(src, tgt, cand, G, params, want_weight=want_weight, method=method)
        return out if want_weight else (lambda: (out(),))


for _G in (1, 6, 11, 12):
    for _w in (False, True):
        _cpg_case(_G, _w)
_cpg_case(6, True, "tiled")            # one block of the tiled kernel
_cpg_case(19, False)                   # 2 x 2 x 2 conv1 blocks, 3 x 3 x 3 conv2 blocks (ops._cpg_blocks)


def _cpg_bwd_case(G, tiled, contiguous=False, ws_keypoints=None):
    name = "cpg_tiled_backward" if tiled else "cpg_backward"
    tag = f"G={G}" + (",contiguous" if contiguous else "") + (f",ws for {ws_keypoints}" if ws_keypoints else "")

    @case(f"{name}[{tag}]")
    def build(cuda):
        from dvcp import _lib, ops
        B, K = 1, 5
        src, tgt, cand, gv = _cpg_inputs(cuda, G, B, K)
        if contiguous:
            tgt = tgt.contiguous()
        params = _cpg_module(cuda).packed_params()
        if not tiled:
            return lambda: ops.cpg_backward(src, tgt, cand, G, params, gv)
        ws_bytes = None
        if ws_keypoints:   # a workspace for fewer key points: chunks (test_cpg_tiled_backward_chunks_and_determinism)
            size = _lib.load().dvcp_cpg_tiled_backward_workspace_bytes
            partials = lambda P: (P * ops.CPG_NPARAMS + 3) // 4 * 16   # noqa: E731
            ws_bytes = partials(B * K) + ws_keypoints * (int(size(1, G)) - partials(1))
        return lambda: ops.cpg_tiled_backward(src, tgt, cand, G, params, gv, ws_bytes=ws_bytes)


_cpg_bwd_case(2, False)
_cpg_bwd_case(6, False)
_cpg_bwd_case(11, False)
_cpg_bwd_case(12, True)
_cpg_bwd_case(12, True, contiguous=True)
_cpg_bwd_case(12, True, ws_keypoints=2)        # five key points: three chunks, the last one short
_cpg_bwd_case(6, True)


# ---- pose --------------------------------------------------------------------------------------
def _pose_inputs(cuda, B=3, n=64, seed=1800):
    from dvcp.synthetic import make_pairs
    g = _g(seed)
    _, _, R_gt, t_gt = make_pairs(B, 8, seed=seed)
    x = torch.rand(B, 3, n, generator=g, dtype=torch.float64) * 2 - 1
    y = torch.matmul(R_gt.double().expand(B, 3, 3), x) + t_gt.double().reshape(-1, 3, 1)
    y = y + 0.05 * torch.randn(B, 3, n, generator=g, dtype=torch.float64)
    w = torch.rand(B, n, generator=g, dtype=torch.float64) + 0.05
    Rt = R_gt.double().expand(B, 3, 3).contiguous()
    tt = t_gt.double().reshape(-1, 3, 1).expand(B, 3, 1).contiguous()
    return x.to(cuda), y.to(cuda), w.to(cuda), Rt.to(cuda), tt.to(cuda)


@case("rigid_transform")
def _(cuda):
    from dvcp import ops
    x, y, _, _, _ = _pose_inputs(cuda)
    return lambda: ops.rigid_transform(x, y)


@case("svd_optimization+backward")
def _(cuda):
    from dvcp import ops
    x, y, _, Rt, tt = _pose_inputs(cuda)
    gl = torch.tensor(0.7, dtype=torch.float64, device=cuda)

    def run():
        out = ops.svd_optimization(x, y, Rt, tt)
        return out + (ops.svd_optimization_backward(x, y, Rt, tt, out[4], gl, 0.5),)
    return run


@case("deepvcp_loss")
def _(cuda):
    from dvcp import ops
    x, y, _, Rt, tt = _pose_inputs(cuda)
    return lambda: ops.deepvcp_loss(x, y, Rt, tt, 0.5)


@case("registration_error")
def _(cuda):
    from dvcp import ops
    _, _, _, Rt, tt = _pose_inputs(cuda, B=37)
    _, _, _, Rp, tp = _pose_inputs(cuda, B=37, seed=1801)
    return lambda: ops.registration_error(Rp, tp, Rt, tt) + ops.registration_error(Rp, tp, Rt[:1], tt[:1])


def _rigid_apply_case(C, per_batch):
    @case(f"rigid_apply[C={C},t={'batch' if per_batch else 'broadcast'}]")
    def build(cuda):
        from dvcp import ops
        g = _g(1810 + C)
        pts = torch.randn(3, C, 777, generator=g).to(cuda)
        _, _, _, R, t = _pose_inputs(cuda)
        tt = t if per_batch else t[:1]
        return lambda: (ops.rigid_apply(pts, R, tt), ops.rigid_apply(pts, R, None))


for _C in (3, 6):
    for _pb in (False, True):
        _rigid_apply_case(_C, _pb)


def _paper_pose_case(ratio):
    @case(f"paper_pose+backward[inlier_ratio={ratio}]")
    def build(cuda):
        from dvcp import ops
        x, y, w, Rt, tt = _pose_inputs(cuda, B=5)
        gl = torch.tensor(1.3, dtype=torch.float64, device=cuda)

        def run():
            R, t = ops.paper_pose(x, y, None, True, ratio)
            R2, t2, partial = ops.paper_pose(x, y, w, True, ratio, Rt, tt)
            gy, gw = ops.paper_pose_backward(x, y, w, Rt, tt, 0.5, gl, True, ratio)
            gy0, _ = ops.paper_pose_backward(x, y, None, Rt, tt, 0.5, gl, False, ratio)
            return R, t, R2, t2, partial, gy, gw, gy0
        return run


_paper_pose_case(1.0)
_paper_pose_case(0.8)


# ---- backward of the extractor (eval-mode BN) and its head ---------------------------------------
def _bwd_sa_inputs(cuda, table, normals=False, point_major=False, B=2, N=600, S=130, seed=1900):
    """One REF-R table at its reference radius and nsample on a cloud dense enough to fill some groups:
    (module, xyz (B, 3, N), centres, feat (B, D, N) view or None, count, list, nsample, grad_out)."""
    import dvcp.pointnet2_utils as P
    from dvcp import ops
    from dvcp.deep_feat_extraction import fe_config
    from tests_helpers import randomize_bn
    cfg = fe_config(use_normal=normals, npoint=S)[table]
    g = _g(seed + table)
    torch.manual_seed(seed + table)
    sa = P.PointNetSetAbstraction(**cfg)
    randomize_bn(sa)
    sa = sa.to(cuda)
    r, D = cfg["radius"], cfg["in_channel"] - 3
    xyz = (_cloud(g, B, N) * 3 * r).transpose(1, 2).contiguous().to(cuda)
    feat = None
    if D:
        feat = torch.randn(B, N, D, generator=g).to(cuda).transpose(1, 2)    # point-major memory
        if not point_major:
            feat = feat.contiguous()                                         # channel-first memory
    start = torch.randint(0, N, (B,), generator=g).to(cuda)
    ns = min(cfg["nsample"], N)
    _, ctr = ops.fps(xyz, S, start, pdim=2)
    count, lst, _ = ops.ball_query(xyz, ctr, r, ns, pdim=2, cdim_pts=2)
    go = torch.randn(B, S, cfg["mlp"][-1], generator=g).to(cuda)
    return sa, xyz, ctr, feat, count, lst, ns, go


def _sa_bwd_case(table):
    @case(f"sa_group_mlp_backward[sa{table + 1}]")
    def build(cuda):
        from dvcp import autograd, ops
        sa, xyz, ctr, feat, count, lst, ns, go = _bwd_sa_inputs(cuda, table)
        sa.eval()
        params, bnstat = sa.packed_params(), autograd._bn_stats(sa)
        return lambda: ops.sa_group_mlp_backward(xyz, ctr, feat, count, lst, ns, sa.chans, params, bnstat, go,
                                                 want_feat_grad=feat is not None)


for _table in (0, 1, 2):
    _sa_bwd_case(_table)


@case("fe_head_backward")
def _(cuda):
    from dvcp import ops
    fe, _ = _head_modules(cuda)
    g = _g(1950)
    x, go = torch.randn(1001, 64, generator=g).to(cuda), torch.randn(1001, 32, generator=g).to(cuda)
    return lambda: ops.fe_head_backward(x, fe.fc_params(), go)


# ---- batch-statistics BatchNorm: the set abstraction ---------------------------------------------
def _sa_bn_case(name, table, mfma, normals=False, point_major=False, keep_zrows=True):
    """batchnorm.train_forward + train_backward on one table: the lane-per-entry passes (dvcp_sa_bn_stats /
    _zrows / _backward) or the matrix-core ones (dvcp_sa_bnm_pre / _pass); the backward reads the forward's
    state (pack, z rows or U and the routing)."""
    @case(name)
    def build(cuda):
        from dvcp import batchnorm
        sa, xyz, ctr, feat, count, lst, ns, go = _bwd_sa_inputs(cuda, table, normals, point_major, seed=2000)
        sa.train()
        want_feat = feat is not None and feat.shape[1] in (32, 64)

        def run():
            keep, batchnorm.USE_MFMA = batchnorm.USE_MFMA, mfma
            try:
                out, st = batchnorm.train_forward(sa, xyz, ctr, feat, count, lst, ns, keep_zrows=keep_zrows)
                assert bool(st.get("mfma")) == mfma
                lay = dict(pts=xyz, ctr=ctr, feat=feat, count=count, lst=lst, ns=ns, bn=st)
                gp, gF = batchnorm.train_backward(sa, lay, go, want_feat_grad=want_feat)
            finally:
                batchnorm.USE_MFMA = keep
            return out, st["pack"], gp, gF
        return run


_sa_bn_case("sa_bn[sa1,valu]", 0, False)                    # 2 x 130 x 256 entries: two 65536-entry chunks
_sa_bn_case("sa_bn[sa1,normals,valu]", 0, False, normals=True)
_sa_bn_case("sa_bn[sa2,valu,zrows kept]", 1, False)
_sa_bn_case("sa_bn[sa2,valu,zrows recomputed]", 1, False, keep_zrows=False)
_sa_bn_case("sa_bn[sa3,valu]", 2, False)
_sa_bn_case("sa_bnm[sa1]", 0, True)
_sa_bn_case("sa_bnm[sa2]", 1, True, point_major=True)
_sa_bn_case("sa_bnm[sa3]", 2, True, point_major=True)


# ---- paper mode ----------------------------------------------------------------------------------
FP_TABLES = [(700, 32, 64, (32, 32)), (700, 0, 32, (32, 32, 32)), (3, 64, 64, (64, 64)), (1, 0, 32, (16,))]


def _fp_inputs(cuda, N2, D1, D2, mlp, bn_train, N1=333, B=2):
    import dvcp
    g = _g(2100 + N2 + D1)
    torch.manual_seed(2100 + N2 + D1)
    fp = dvcp.paper.PointNetFeaturePropagation(D1 + D2, list(mlp), bn_train=bn_train)
    with torch.no_grad():
        for bn in fp.mlp_bns:
            n = bn.num_features
            bn.weight.copy_(torch.rand(n, generator=g) + 0.5)
            bn.bias.copy_(torch.rand(n, generator=g) * 0.2 - 0.1)
            bn.running_mean.copy_(torch.rand(n, generator=g) * 0.2 - 0.1)
            bn.running_var.copy_(torch.rand(n, generator=g) + 0.5)
    fp = fp.to(cuda).train(bn_train)
    xyz1 = _cloud(g, B, N1).transpose(1, 2).contiguous().to(cuda)
    xyz2 = _cloud(g, B, N2).transpose(1, 2).contiguous().to(cuda)
    p1 = torch.randn(B, D1, N1, generator=g).to(cuda) if D1 else None
    p2 = torch.randn(B, N2, D2, generator=g).to(cuda)
    go = torch.randn(B, N1, mlp[-1], generator=g).to(cuda)
    return fp, xyz1, xyz2, p1, p2, go


def _fp_case(N2, D1, D2, mlp):
    @case(f"feature_propagation+backward[N2={N2},D1={D1}]")
    def build(cuda):
        from dvcp import ops
        fp, xyz1, xyz2, p1, p2, go = _fp_inputs(cuda, N2, D1, D2, mlp, False)
        packed = fp.packed_params()
        bnstat = torch.cat([t for bn in fp.mlp_bns
                            for t in (bn.running_mean.float(), torch.rsqrt(bn.running_var.double() + bn.eps).float())])
        relu = [1] * len(mlp)

        def run():
            out = ops.feature_propagation(xyz1, xyz2, p2, p1, fp.chans, relu, packed)
            return (out,) + ops.feature_propagation_backward(xyz1, xyz2, p2, p1, fp.chans, relu, packed, bnstat, go)
        return run

    @case(f"feature_propagation_bn[N2={N2},D1={D1}]")
    def build_bn(cuda):
        from dvcp import batchnorm
        fp, xyz1, xyz2, p1, p2, go = _fp_inputs(cuda, N2, D1, D2, mlp, True)

        def run():   # dvcp_feature_propagation_bn_stats, the forward, dvcp_feature_propagation_bn_backward
            out, st = batchnorm.fp_train_forward(fp, xyz1, xyz2, p1, p2)
            return (out, st["pack"], st["bnstat"]) + batchnorm.fp_train_backward(st, xyz1, xyz2, p1, p2, go)
        return run


for _t in FP_TABLES:
    _fp_case(*_t)


def _group_rows_case(N, ns):
    @case(f"group_rows+backward[N={N},nsample={ns}]")
    def build(cuda):
        from dvcp import ops
        g = _g(2200 + N)
        B, Q = 2, 300
        xyz = _cloud(g, B, N).to(cuda)
        feat = torch.randn(B, N, 32, generator=g).to(cuda)
        ctr = (torch.rand(B, Q, 3, generator=g) * 6 - 3).to(cuda)       # most centres far outside: empty balls
        cnt, lst, _ = ops.ball_query(xyz, ctr, 0.5, min(ns, N), pdim=1, cdim_pts=1)
        assert bool((cnt == 0).any()) and bool((cnt > 0).any())
        go = torch.randn(B, Q, ns, 35, generator=g).to(cuda)
        return lambda: (ops.group_rows(ctr, xyz, feat, cnt, lst, ns, 0.5, ctr_pdim=1, xyz_pdim=1),
                        ops.group_rows(ctr, xyz, None, cnt, lst, ns, 0.5, ctr_pdim=1, xyz_pdim=1),
                        ops.group_rows_backward(cnt, lst, ns, N, go))


_group_rows_case(2000, 32)
_group_rows_case(20, 32)               # nsample above the cloud size: padding with the first hit


def _cpg1d_case(Gz):
    @case(f"cpg1d+backward[Gz={Gz}]")
    def build(cuda):
        import dvcp
        from dvcp import ops
        g = _g(2300 + Gz)
        torch.manual_seed(2300)
        params = dvcp.paper.CPG1D().eval().to(cuda).packed_params()
        B, K = 2, 37
        src = torch.randn(B, K, 32, generator=g).to(cuda)
        tgt = torch.randn(B, K, Gz, 32, generator=g).to(cuda)
        cand = torch.randn(B, K, Gz, 3, generator=g).to(cuda)
        gv = torch.randn(B, K, 3, generator=g).to(cuda)

        def run():
            vcp, w = ops.cpg1d(src, tgt, cand, params, want_weight=True)
            return (vcp, w, ops.cpg1d(src, tgt, cand, params)) + ops.cpg1d_backward(src, tgt, cand, params, gv) \
                + ops.cpg1d_backward(src, tgt, cand, params, gv, want_src=False, want_tgt=False)
        return run


for _Gz in (1, 9, 64):
    _cpg1d_case(_Gz)


def _paper_wl(cuda, bn_train):
    import dvcp
    torch.manual_seed(2400)
    wl = dvcp.paper.PaperWeighting(bn_train=bn_train).to(cuda)
    return wl.train(bn_train)


def _wl_case(P):
    @case(f"weighting_backward[P={P}]")
    def build(cuda):
        from dvcp import ops
        g = _g(2400 + P)
        params = _paper_wl(cuda, False).packed_params()
        feat, gs = torch.randn(P, 32, generator=g).to(cuda), torch.randn(P, generator=g).to(cuda)
        return lambda: (ops.weighting(feat, params),) + ops.weighting_backward(feat, params, gs) \
            + ops.weighting_backward(feat, params, gs, want_feat=False)

    @case(f"weighting_bn[P={P}]")
    def build_bn(cuda):
        from dvcp import batchnorm
        g = _g(2400 + P)
        wl = _paper_wl(cuda, True)
        feat, gs = torch.randn(P, 32, generator=g).to(cuda), torch.randn(P, generator=g).to(cuda)

        def run():   # dvcp_weighting_bn_stats, _forward, _backward (modes 2, 1, 0)
            score, st = batchnorm.weighting_train_forward(wl, feat)
            grads, gfeat = batchnorm.weighting_train_backward(wl, st, gs, True)
            return score, st["pack"], st["bnstat"], grads, gfeat
        return run


_wl_case(1001)
_wl_case(2)


# ---- empty inputs --------------------------------------------------------------------------------
# No row, centre or key point: the backward launchers return before any kernel and fill what they promise with
# a hipMemsetAsync (zero sums and parameter gradients) -- the only initialisation those outputs get.  (The
# forward launchers refuse the null pointers of torch's empty tensors and have nothing to write; so do the
# set-abstraction backward entry points, whose empty paths the wrappers therefore never reach.)

@case("empty[dfe_backward,cpg_backward,dfe_tgt_backward]")
def _(cuda):
    from dvcp import ops   # the calls of test_gpu_train.py::test_backward_entry_points_empty_inputs
    g = _g(2500)
    params, cparams = _dfe_module(cuda).packed_params(), _cpg_module(cuda).packed_params()
    z = lambda *shape, **kw: torch.zeros(*shape, device=cuda, **kw)   # noqa: E731
    B, M, C = 2, 500, 216
    ref_xyz, feat = torch.rand(B, 3, M, generator=g).to(cuda), torch.rand(B, M, 32, generator=g).to(cuda)
    return lambda: (ops.dfe_backward(z(0, 32, 35), params, z(0, 32)),
                    ops.cpg_backward(z(0, 2, 32), z(0, 2, 32, C), z(0, 2, C, 3), 6, cparams, z(0, 2, 3)),
                    ops.cpg_tiled_backward(z(0, 2, 32), z(0, 2, 32, 1728), z(0, 2, 1728, 3), 12, cparams, z(0, 2, 3)),
                    ops.dfe_tgt_backward(ref_xyz, feat, z(B, 0, 3), z(B, 0, 32), z(B, 0, 32, dtype=torch.int32), params,
                                         z(B, 0, 32), want_feat_grad=True))


@case("empty[weighting,P=0]")
def _(cuda):
    from dvcp import ops
    g = _g(2510)
    params = _paper_wl(cuda, False).packed_params()
    pack = torch.randn(ops.WEIGHTING_BN_NPARAMS, generator=g).to(cuda)
    bnstat = torch.rand(ops.WEIGHTING_BN_NSTAT, generator=g, dtype=torch.float64).to(cuda)
    feat, gs = torch.zeros(0, 32, device=cuda), torch.zeros(0, device=cuda)
    return lambda: (ops.weighting_backward(feat, params, gs),
                    ops.weighting_bn_stats(feat, pack, 1), ops.weighting_bn_stats(feat, pack, 2),
                    ops.weighting_bn_backward(feat, pack, bnstat, gs, 2),
                    ops.weighting_bn_backward(feat, pack, bnstat, gs, 1),
                    ops.weighting_bn_backward(feat, pack, bnstat, gs, 0))


@case("empty[cpg1d,P=0]")
def _(cuda):
    import dvcp
    from dvcp import ops
    torch.manual_seed(2300)
    params = dvcp.paper.CPG1D().eval().to(cuda).packed_params()
    z = lambda *shape: torch.zeros(*shape, device=cuda)   # noqa: E731
    return lambda: (ops.cpg1d_backward(z(0, 4, 32), z(0, 4, 9, 32), z(0, 4, 9, 3), params, z(0, 4, 3)))


@case("empty[feature_propagation,N1=0]")
def _(cuda):
    from dvcp import ops
    N2, D1, D2, mlp = FP_TABLES[0]
    fp, _, xyz2, _, p2, _ = _fp_inputs(cuda, N2, D1, D2, mlp, False)
    B, chans, relu = 2, fp.chans, [1] * len(mlp)
    packed = fp.packed_params()
    g = _g(2520)
    bnstat = torch.rand(2 * sum(chans[1:]), generator=g).to(cuda)
    bnstat64 = torch.rand(4 * sum(chans[1:]), generator=g, dtype=torch.float64).to(cuda)
    xyz1, p1 = (torch.zeros(B, c, 0, device=cuda) for c in (3, D1))
    go = torch.zeros(B, 0, chans[-1], device=cuda)
    return lambda: (ops.feature_propagation_backward(xyz1, xyz2, p2, p1, chans, relu, packed, bnstat, go),
                    ops.feature_propagation_bn_stats(xyz1, xyz2, p2, p1, chans, relu, packed, 1),
                    ops.feature_propagation_bn_backward(xyz1, xyz2, p2, p1, chans, relu, packed, bnstat64, go, 2),
                    ops.feature_propagation_bn_backward(xyz1, xyz2, p2, p1, chans, relu, packed, bnstat64, go, 0))


@case("empty[group_rows_backward,Q=0]")
def _(cuda):
    from dvcp import ops
    cnt = torch.zeros(2, 0, dtype=torch.int32, device=cuda)
    lst = torch.zeros(2, 0, 32, dtype=torch.int32, device=cuda)
    go = torch.zeros(2, 0, 32, 35, device=cuda)
    return lambda: (ops.group_rows_backward(cnt, lst, 32, 77, go),)


# ------------------------------------------------------------------------------------------------
# the runner

@contextlib.contextmanager
def _logging_calls():
    """Log the entry-point names that go through ``_lib.call`` and the name ``ops`` bound it to."""
    from dvcp import _lib, ops
    real = _lib.call

    def spy(name, *args, **kw):
        SEEN.add(name)
        return real(name, *args, **kw)

    keep = (_lib.call, ops.call)
    _lib.call = ops.call = spy
    try:
        yield
    finally:
        _lib.call, ops.call = keep


@contextlib.contextmanager
def _stop_on_gpu_error(name):
    """A poisoned run may fault instead of differing (a kernel that consumed an uninitialised index).  After a
    device error nothing more is started on the GPU: the session ends here instead of failing test after test."""
    try:
        yield
    except RuntimeError as e:
        text = str(e).lower()
        if "hip error" in text or "illegal memory access" in text or "device-side" in text or "hiperror" in text:
            pytest.exit(f"{name}: device error, no further GPU work in this session: {e}", returncode=3)
        raise


def _flatten(out):
    if out is None or isinstance(out, torch.Tensor):
        return [out]
    assert isinstance(out, (tuple, list)), type(out)
    return [t for o in out for t in _flatten(o)]


def _finish():
    from dvcp import _lib
    torch.cuda.synchronize()
    _lib.check_device_flags(block=True)


def _compare(name, what, got, want, tol=None):
    """Bit identity of two flattened output lists (tensors on the CPU); with ``tol`` = (output index, bound), that
    one output is held to the parity test's max |a - b| <= bound max |b| instead, NaNs in the same places."""
    assert len(got) == len(want), (name, what)
    for i, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), (name, what, i)
        if a is None:
            continue
        assert a.shape == b.shape and a.dtype == b.dtype, (name, what, i, a.shape, b.shape)
        if torch.equal(bits(a), bits(b)):
            continue
        if tol is not None and i == tol[0]:
            a64, b64 = a.double(), b.double()
            assert torch.equal(torch.isnan(a64), torch.isnan(b64)), (name, what, i, "NaNs moved")
            err = float((a64 - b64).nan_to_num(0.0).abs().max())
            scale = float(b64.nan_to_num(0.0).abs().max())
            print(f"{name}: {what}: output {i} differs in bits, max |a - b| {err:.3e} of {scale:.3e} (bound {tol[1]})")
            assert err <= tol[1] * scale, f"{name}: {what}, output {i}: max |a - b| {err:.3e} > {tol[1]} x {scale:.3e}"
            continue
        diff = (bits(a) != bits(b)).nonzero()
        first = int(diff[0]) // a.element_size()
        raise AssertionError(f"{name}: {what}: output {i} {tuple(a.shape)} {a.dtype} differs in "
                             f"{diff.numel()} bytes, first at element {first}: "
                             f"{a.reshape(-1)[first].item()!r} vs {b.reshape(-1)[first].item()!r}")


def _four_runs(name, run, mask=None, tol=None):
    """plain, plain, 0xFF, 0x5A -> the plain outputs; asserts the module docstring's rules."""
    def snap(out):
        out = mask(out) if mask is not None else out
        _finish()
        return [None if t is None else t.detach().cpu() for t in _flatten(out)]

    with _logging_calls(), _stop_on_gpu_error(name):
        plain = snap(run())
        again = snap(run())
        _compare(name, "the second plain run against the first" + ("" if tol is None else " (within the tolerance)"),
                 again, plain, tol)
        for byte in POISONS:
            with Poison(byte) as mc:
                out = run()
            damaged = mc.check()
            assert mc.blocks, f"{name}: no allocation went through the hook"
            assert all(big.data_ptr() % 512 == 0 for _, big, _, _, _ in mc.blocks)
            assert damaged == [], f"{name}: under 0x{byte:02X} guard bytes were overwritten: {damaged}"
            _compare(name, f"the run under 0x{byte:02X} against the plain run", snap(out), plain, tol)
    return plain


@pytest.mark.parametrize("name", list(CASES))
def test_entry_point_under_poison(cuda, name):
    run = CASES[name](cuda)
    tol = NOT_BIT_REPRODUCIBLE[name][:2] if name in NOT_BIT_REPRODUCIBLE else None
    _four_runs(name, run, UNSPECIFIED.get(name), tol)
    _RAN.add(name)


def test_exception_lists_name_cases():
    assert set(NOT_BIT_REPRODUCIBLE) <= set(CASES) and set(UNSPECIFIED) <= set(CASES)


# ------------------------------------------------------------------------------------------------
# composite passes: the allocation sites of autograd.py, batchnorm.py, paper.py and the extractor
# (deep_feat_extraction.py, its side stream included)

def _grads(model):
    return [p.grad for _, p in sorted(model.named_parameters())]


def test_composite_eval_forward(cuda):
    """DeepVCP in eval mode on the e2e_c1 fixture: forward + deepVCP_loss."""
    import test_gpu_e2e as E
    from tests_helpers import golden
    z = golden("e2e_c1")
    model = E._load_model(cuda, z)

    def run():
        _, kp, vcp, loss, R, t = E._forward(cuda, model, z)
        return kp, vcp, loss, R, t
    _four_runs("DeepVCP eval forward (e2e_c1)", run)


def test_composite_head_train_step(cuda):
    """test_gpu_train.py::test_head_train_step_vs_oracle's model and size (K = 32, r = 1.0, s = 0.4, 512
    extractor points, one pair of 1024 points, the extractor frozen in eval mode): forward, loss, backward."""
    import dvcp
    from dvcp.synthetic import make_pairs, randomize_bn
    src, tgt, R_gt, t_gt = (t.to(cuda) for t in make_pairs(1, 1024, seed=91))
    torch.manual_seed(0)
    model = dvcp.DeepVCP(use_normal=False, K=32, r=1.0, s=0.4, fe_npoint=512)
    randomize_bn(model)
    model.to(cuda)
    model.FE1.eval()
    model.FE1.requires_grad_(False)
    starts = model.draw_starts(1, 1024, 1024)

    def run():
        model.zero_grad(set_to_none=True)
        kp, vcp = model(src, tgt, R_gt, torch.zeros(1, 3), starts=starts)
        loss, R, t = dvcp.deepVCP_loss(kp, vcp, R_gt, t_gt, 0.5)
        loss.backward()
        grads = _grads(model)
        assert sum(g is not None for g in grads) >= 12
        return kp, vcp.detach(), loss.detach(), R, t, grads
    _four_runs("DeepVCP head-training step", run)


def test_composite_paper_train_step(cuda):
    """DeepVCPPaper(train_extractor=True, bn_train=True) in train(): one step (forward, the paper loss over
    both stages, backward) at npoints (512, 128, 32), K = 16, N = 2048.  Batch statistics do not read the
    running ones, so the four runs see the same state."""
    import dvcp
    from dvcp.synthetic import make_pairs
    B, N = 2, 2048
    src, tgt, R_gt, t_gt = (t.to(cuda) for t in make_pairs(B, N, seed=92))
    torch.manual_seed(2)
    model = dvcp.paper.DeepVCPPaper(use_normal=False, K=16, r=0.4, s=0.4, s_z=0.25, d=1.0, npoints=(512, 128, 32),
                                    train_extractor=True, bn_train=True).to(cuda).train()
    torch.manual_seed(3)
    starts = torch.stack([model.FE.draw_starts(B, N), model.FE.draw_starts(B, N)])

    def run():
        model.zero_grad(set_to_none=True)
        got = model(src, tgt, R_gt, torch.zeros(1, 3), starts=starts)
        loss = 0.0
        for st in got:
            loss = loss + dvcp.paper.deepVCP_loss_paper(st["keypts"], st["vcp"], st["weights"], R_gt, t_gt, 0.5,
                                                        inlier_ratio=0.8)[0]
        loss.backward()
        grads = _grads(model)
        assert all(g is not None for g in grads)
        return [(st["keypts"], st["vcp"].detach(), st["weights"].detach(), st["R"], st["t"]) for st in got], \
            loss.detach(), grads
    _four_runs("DeepVCPPaper train step", run)


# ------------------------------------------------------------------------------------------------
# the coverage gate

# entry points (dvcp/_lib.py SIGNATURES) that no case runs, each with its reason
EXCLUDED = {
    "dvcp_fps_step_floor": "a timing probe of the benchmark (an empty step loop): one word of output, no product path",
    "dvcp_fps_split_probe": "a test probe that withholds workgroups so that the split kernel's guard must fire "
                            "(tests/test_gpu_configs.py): its result is the error word, not FPS indices",
    "dvcp_knn_tiled_order_probe": "a test probe that dumps the tiled kNN's visiting order "
                                  "(tests/test_gpu_knn_order.py); dvcp_knn_tiled runs the same build and order kernels",
}
# exported symbols outside SIGNATURES: host-side queries that launch nothing and touch no device memory
EXCLUDED_SUFFIXES = {
    "_workspace_bytes": "a size query answered on the host",
    "_floats": "a size query answered on the host",
    "_supported": "a capability query answered on the host",
    "_nparams": "a size query answered on the host",
}
EXCLUDED_HOST = {"dvcp_abi_version": "returns a constant", "dvcp_last_error": "returns the host's last error string"}


def test_every_entry_point_has_a_case(cuda):
    """Every exported symbol is reached by a case or excluded with a reason; a new entry point fails here
    until it has a case.  Cases that this session did not run (a -k selection) run once, plain."""
    from dvcp import _lib
    with _logging_calls():
        for name in CASES:
            if name not in _RAN:
                CASES[name](cuda)()
                _finish()
                _RAN.add(name)
    assert all(reason for reason in list(EXCLUDED.values()) + list(EXCLUDED_SUFFIXES.values()))
    assert set(EXCLUDED) <= set(_lib.SIGNATURES) and not set(EXCLUDED) & SEEN

    def excluded(name):
        return name in EXCLUDED or name in EXCLUDED_HOST or (name not in _lib.SIGNATURES
                                                             and name.endswith(tuple(EXCLUDED_SUFFIXES)))
    names = set(_lib.exported_symbols()) | set(_lib.SIGNATURES)
    missing = sorted(n for n in names if n not in SEEN and not excluded(n))
    assert not missing, f"entry points without a memcheck case: {missing}"
