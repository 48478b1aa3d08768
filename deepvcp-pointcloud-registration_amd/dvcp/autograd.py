"""Autograd for the registration head: training drop-in for train.py:105-125.

The reference trains with ``loss.backward()`` through deepVCP_loss (two torch.svd), the corresponding
point generation (cpg.py), the deep feature embedding (deep_feat_embedding.py, src and tgt) and the
feature extractor.  Here the head's backward runs in hand-written HIP kernels:

  * ``pose_loss``  -- deepVCP_loss.py:105-121 forward (dvcp_svd_optimization) and backward
                      (dvcp_svd_optimization_backward, both Kabsch solves differentiated);
  * ``cpg``        -- cpg.py:27-60 (dvcp_cpg / dvcp_cpg_backward; G > 11: the tiled pair): gradients for the conv
                      weights and for both DFE outputs;
  * ``dfe_rows``   -- deep_feat_embedding.py on the source rows (dvcp_dfe / dvcp_dfe_backward);
  * ``dfe_tgt``    -- the fused target rows (dvcp_dfe_tgt / dvcp_dfe_tgt_backward), also
                      differentiable in the target features (the get_cat_feat_tgt.py:85 gather);
  * ``src_keypoints`` -- the key-point stage, differentiable in the source features (the
                      pointnet2_utils.py:59 gather, dvcp_src_keypoints_backward; above 256 key
                      points dvcp_src_keypoints_backward_ws on the forward's workspace).

  * ``feat_extraction`` -- the feature extractor (deep_feat_extraction.py:18-32 + REF-R R1): fc
                      (dvcp_fe_head_backward) and the three set-abstraction MLPs, chained through the
                      FPS-order gathers and the ball-query groupings.  BatchNorm in eval mode
                      (frozen-BN training, FE1.eval()): dvcp_sa_group_mlp_backward; in training mode
                      (batch statistics, model.train() as train.py does): dvcp_sa_bn_backward
                      (dvcp/batchnorm.py).

Paper mode (dvcp/paper.py, not reference parity) adds the two links its stage heads need:

  * ``cpg1d``      -- the second stage's 1-D CPG (dvcp_cpg1d / dvcp_cpg1d_backward);
  * ``weighting``  -- the paper's weighting layer (dvcp_weighting / dvcp_weighting_backward), whose
                      scores are the pose solve's weights there and so do carry a gradient;
  * ``weighting_bn`` -- the same layer in training mode, batch-statistics BN (dvcp_weighting_bn_stats /
                      _forward / _backward through dvcp/batchnorm.py);

and the links that train its extractor (``DeepVCPPaper(train_extractor=True)``):

  * ``feature_propagation`` -- PointNetFeaturePropagation (dvcp_feature_propagation /
                      dvcp_feature_propagation_backward: the 3-NN and the layer chain recomputed);
  * ``group_rows`` -- the DFE rows' gather (dvcp_group_rows / dvcp_group_rows_backward);
  * ``paper_feat_extraction`` -- PaperFeatExtraction: the three set abstractions (dvcp_sa_group_mlp /
                      dvcp_sa_group_mlp_backward) and the three propagations, composed per layer.

The key points, candidates and kNN indices carry no gradient in the reference either (index
ops, knn_cuda under no_grad); the reference path's weighting layer gets none (only its top-k
indices are used).
Parameter gradients come back summed over
the batch in a fixed order (deterministic); the feature scatters use float atomics.
"""
import torch

from . import batchnorm, ops


def _pack(weights):
    return torch.cat([w.detach().reshape(-1) for w in weights]).float().contiguous()


def _split(gp, weights):
    """Packed gradient -> one tensor per (shape, dtype) in ``weights``."""
    out, o = [], 0
    for shape, dtype in weights:
        n = shape.numel()
        out.append(gp[o:o + n].view(shape).to(dtype))
        o += n
    return out


class _DfeRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, *weights):
        params = _pack(weights)
        ctx.save_for_backward(X, params)
        ctx.weights = [(w.shape, w.dtype) for w in weights]
        return ops.dfe(X, params)

    @staticmethod
    def backward(ctx, g):
        X, params = ctx.saved_tensors
        if ctx.needs_input_grad[0]:
            gp, gX = ops.dfe_backward(X, params, g, want_input_grad=True)
            return (gX.to(X.dtype), *_split(gp, ctx.weights))
        return (None, *_split(ops.dfe_backward(X, params, g), ctx.weights))


class _DfeTgt(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ref_xyz, ref_feat, cand, dist, idx, *weights):
        params = _pack(weights)
        ctx.save_for_backward(ref_xyz, ref_feat, cand, dist, idx, params)
        ctx.weights = [(w.shape, w.dtype) for w in weights]
        return ops.dfe_tgt(ref_xyz, ref_feat, cand, dist, idx, params, ref_pdim=2)

    @staticmethod
    def backward(ctx, g):
        ref_xyz, ref_feat, cand, dist, idx, params = ctx.saved_tensors
        if ctx.needs_input_grad[1]:  # the get_cat_feat_tgt.py:85 gather's backward
            gp, gF = ops.dfe_tgt_backward(ref_xyz, ref_feat, cand, dist, idx, params, g, ref_pdim=2,
                                          want_feat_grad=True)
            return (None, gF.to(ref_feat.dtype), None, None, None, *_split(gp, ctx.weights))
        gp = ops.dfe_tgt_backward(ref_xyz, ref_feat, cand, dist, idx, params, g, ref_pdim=2)
        return (None, None, None, None, None, *_split(gp, ctx.weights))


class _Cpg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, tgt, cand, G, *weights):
        params = _pack(weights)
        ctx.save_for_backward(src, tgt, cand, params)
        ctx.G = G
        ctx.method = ops.cpg_method(G)
        ctx.weights = [(w.shape, w.dtype) for w in weights]
        return ops.cpg(src, tgt, cand, G, params)

    @staticmethod
    def backward(ctx, g):
        src, tgt, cand, params = ctx.saved_tensors
        backward = ops.cpg_backward if ctx.method == "lds" else ops.cpg_tiled_backward
        gsrc, gtgt, gp = backward(src, tgt, cand, ctx.G, params, g)
        gsrc = gsrc.view(src.shape).to(src.dtype) if ctx.needs_input_grad[0] else None
        gtgt = gtgt.to(tgt.dtype) if ctx.needs_input_grad[1] else None
        return (gsrc, gtgt, None, None, *_split(gp, ctx.weights))


class _Cpg1d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, tgt, cand, *weights):
        params = _pack(weights)
        ctx.save_for_backward(src, tgt, cand, params)
        ctx.weights = [(w.shape, w.dtype) for w in weights]
        return ops.cpg1d(src, tgt, cand, params)

    @staticmethod
    def backward(ctx, g):
        src, tgt, cand, params = ctx.saved_tensors
        want_src, want_tgt = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gsrc, gtgt, gp = ops.cpg1d_backward(src, tgt, cand, params, g, want_src=want_src, want_tgt=want_tgt)
        gsrc = gsrc.view(src.shape).to(src.dtype) if want_src else None
        gtgt = gtgt.to(tgt.dtype) if want_tgt else None
        return (gsrc, gtgt, None, *_split(gp, ctx.weights))


class _Weighting(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, folded):
        rows = feat.contiguous().float()
        params = folded.detach().float().contiguous()
        ctx.save_for_backward(rows, params)
        ctx.dtypes = (feat.dtype, folded.dtype)
        return ops.weighting(rows, params)

    @staticmethod
    def backward(ctx, g):
        rows, params = ctx.saved_tensors
        want_feat = ctx.needs_input_grad[0]
        gp, gfeat = ops.weighting_backward(rows, params, g, want_feat=want_feat)
        return (gfeat.to(ctx.dtypes[0]) if want_feat else None,
                gp.to(ctx.dtypes[1]) if ctx.needs_input_grad[1] else None)


class _WeightingBN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, wl, feat, *params):
        rows = feat.contiguous().float()
        score, st = batchnorm.weighting_train_forward(wl, rows)
        ctx.save_for_backward(st["rows"], st["pack"], st["bnstat"])
        ctx.wl, ctx.M, ctx.dtypes = wl, st["M"], (feat.dtype, [p.dtype for p in params])
        return score

    @staticmethod
    def backward(ctx, g):
        want_feat = ctx.needs_input_grad[1]
        rows, pack, bnstat = ctx.saved_tensors
        st = dict(rows=rows, pack=pack, bnstat=bnstat, M=ctx.M)
        grads, gfeat = batchnorm.weighting_train_backward(ctx.wl, st, g, want_feat)
        return (None, gfeat.to(ctx.dtypes[0]) if want_feat else None,
                *[gr.to(dt) if ctx.needs_input_grad[2 + k] else None
                  for k, (gr, dt) in enumerate(zip(grads, ctx.dtypes[1]))])


class _SrcKeypoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fe_xyz, fe_feat, topk_idx, kstart, R_init, radius, nsample):
        ctx.method = ops.src_keypoints_method(topk_idx.shape[1])
        ctx.radius, ctx.nsample, ctx.feat_dtype = radius, nsample, fe_feat.dtype
        if ctx.method == "split":
            # K > 256 (dvcp_src_keypoints_ws): the backward reads the forward's workspace (FPS order,
            # ball lists, key-point coordinates) instead of repeating the serial FPS
            keypts, src_cat, moved, ws = ops.src_keypoints(fe_xyz, fe_feat, topk_idx, kstart, R_init, radius=radius,
                                                           nsample=nsample, return_workspace=True)
            ctx.save_for_backward(ws)
            ctx.S, ctx.K, ctx.xyz_dtype = fe_xyz.shape[2], topk_idx.shape[1], fe_xyz.dtype
        else:
            keypts, src_cat, moved = ops.src_keypoints(fe_xyz, fe_feat, topk_idx, kstart, R_init, radius=radius,
                                                       nsample=nsample)
            ctx.save_for_backward(fe_xyz, topk_idx, kstart)
        ctx.mark_non_differentiable(keypts, moved)
        return keypts, src_cat, moved

    @staticmethod
    def backward(ctx, g_kp, g_cat, g_moved):
        gF = None
        if ctx.needs_input_grad[1] and g_cat is not None:
            if ctx.method == "split":
                ws, = ctx.saved_tensors
                gF = ops.src_keypoints_backward_ws(ws, ctx.S, ctx.K, g_cat, nsample=ctx.nsample,
                                                   dtype=ctx.xyz_dtype).to(ctx.feat_dtype)
            else:
                fe_xyz, topk_idx, kstart = ctx.saved_tensors
                gF = ops.src_keypoints_backward(fe_xyz, topk_idx, kstart, g_cat, radius=ctx.radius,
                                                nsample=ctx.nsample).to(ctx.feat_dtype)
        return None, gF, None, None, None, None, None


class _PoseLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y_pred, R_true, t_true, alpha):
        x, y, Rt, tt = ops.pose_inputs(x, y_pred, R_true, t_true)
        R, t, x1, _, partial = ops.svd_optimization(x, y, Rt, tt)
        denom = float(x1.numel())
        loss = alpha * (partial[:, 0].sum() / denom) + (1 - alpha) * torch.abs(partial[:, 1].sum() / denom)
        ctx.save_for_backward(x, y, Rt, tt, partial)
        ctx.alpha = alpha
        ctx.y_dtype = y_pred.dtype
        ctx.mark_non_differentiable(R, t)
        return loss, R, t

    @staticmethod
    def backward(ctx, g_loss, g_R, g_t):
        x, y, Rt, tt, partial = ctx.saved_tensors
        gy = ops.svd_optimization_backward(x, y, Rt, tt, partial, g_loss, ctx.alpha)
        return None, gy.to(ctx.y_dtype), None, None, None


def _fe_params(fe):
    """FE1's trainable tensors in a fixed order: per SA layer (conv.weight, conv.bias, bn.weight,
    bn.bias) per MLP layer, then fc.weight, fc.bias."""
    out = []
    for sa in (fe.sa1, fe.sa2, fe.sa3):
        for conv, bn in zip(sa.mlp_convs, sa.mlp_bns):
            out += [conv.weight, conv.bias, bn.weight, bn.bias]
    return out + [fe.fc.weight, fe.fc.bias]


def _bn_stats(sa):
    """Per MLP layer: running_mean | 1 / sqrt(running_var + eps) (fp32), the eval-mode BN's
    normalisation for the gamma gradient."""
    parts = []
    for bn in sa.mlp_bns:
        parts += [bn.running_mean.float(), torch.rsqrt(bn.running_var.double() + bn.eps).float()]
    return torch.cat(parts).contiguous()


def _scatter_rows(g, idx, n):
    """The backward of gathering per-point rows by FPS indices: (B, S, C) -> (B, n, C)."""
    out = torch.zeros(g.shape[0], n, g.shape[2], dtype=torch.float32, device=g.device)
    return out.scatter_add_(1, idx.unsqueeze(-1).expand(-1, -1, g.shape[2]), g.float())


class _FeatExtract(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fe, pts, starts, wl, side_stream, fps, *params):
        saved = {}
        xyz, feat, score = fe.run(pts, starts, wl=wl, side_stream=side_stream, saved=saved, fps=fps)
        ctx.fe, ctx.saved = fe, saved
        ctx.shapes = [(p.shape, p.dtype) for p in params]
        ctx.mark_non_differentiable(xyz)
        if score is not None:
            ctx.mark_non_differentiable(score)
        return xyz, feat, score

    @staticmethod
    def backward(ctx, g_xyz, g_feat, g_score):
        fe, saved = ctx.fe, ctx.saved
        grads = []
        if g_feat is None:
            return (None,) * 6 + tuple(None for _ in ctx.shapes)
        B, S, _ = g_feat.shape
        gp_fc, g = ops.fe_head_backward(saved["f3"], fe.fc_params(), g_feat.reshape(B * S, 32))
        g = g.view(B, S, 64)
        per_layer = []
        for sa, lay in reversed(list(zip((fe.sa1, fe.sa2, fe.sa3), saved["layers"]))):
            n_l = lay["pts"].shape[2]
            g_out = _scatter_rows(g, lay["idx"], n_l) if lay["per_point"] else g
            first = sa is fe.sa1
            if lay["bn"] is not None:   # training-mode BN: batch statistics (dvcp/batchnorm.py)
                gp, g_in = batchnorm.train_backward(sa, lay, g_out, want_feat_grad=not first)
            else:
                gp, g_in = ops.sa_group_mlp_backward(lay["pts"], lay["ctr"], lay["feat"], lay["count"], lay["lst"],
                                                     lay["ns"], sa.chans, sa.packed_params(), _bn_stats(sa), g_out,
                                                     want_feat_grad=not first)
            per_layer.append((sa, gp))
            g = g_in  # (B, n_l, D): the previous layer's outputs, in its centre order
        for sa, gp in reversed(per_layer):
            o = 0
            for conv, bn in zip(sa.mlp_convs, sa.mlp_bns):
                co, ci = conv.weight.shape[0], conv.weight.shape[1]
                grads += [gp[o:o + co * ci].view(conv.weight.shape), gp[o + co * ci:o + co * ci + co],
                          gp[o + co * ci + co:o + co * ci + 2 * co], gp[o + co * ci + 2 * co:o + co * ci + 3 * co]]
                o += co * ci + 3 * co
        grads += [gp_fc[:32 * 64].view(32, 64), gp_fc[32 * 64:]]
        ctx.saved = None
        out = [gr.to(dt) if ctx.needs_input_grad[6 + k] else None for k, (gr, (_, dt)) in enumerate(zip(grads, ctx.shapes))]
        return (None, None, None, None, None, None, *out)


def feat_extraction(fe, pts, starts, wl=None, side_stream=None, fps=None):
    """FE1.run differentiable in FE1's parameters (BN in FE1's mode): -> (xyz, feat, score).
    ``fps``: the FPS chain launched ahead (FE1.launch_fps)."""
    return _FeatExtract.apply(fe, pts, starts, wl, side_stream, fps, *_fe_params(fe))


def dfe_rows(X, dfe_module):
    """deep_feat_embedding.py forward on materialised rows (..., 32, 35), differentiable in fc1-3."""
    return _DfeRows.apply(X, *_linears(dfe_module))


def dfe_tgt(ref_xyz, ref_feat, cand, dist, idx, dfe_module):
    """The fused target rows (get_cat_feat_tgt.py + deep_feat_embedding.py), differentiable in fc1-3."""
    return _DfeTgt.apply(ref_xyz, ref_feat, cand, dist, idx, *_linears(dfe_module))


def require_trainable_grid(G, large_grid=False):
    """Grids above 11^3 take the tiled CPG (dvcp_cpg_tiled), whose backward (dvcp_cpg_tiled_backward)
    is opt-in: without ``large_grid`` a forward that records autograd there is refused when it is
    recorded, not in the middle of loss.backward().  With ``large_grid=True`` every G <= 32 passes
    (ValueError above, as ``ops.cpg_method``).  The default is meant to flip to True once the test
    that pins the refusal is retired."""
    if ops.cpg_method(G) != "lds" and not large_grid:
        raise NotImplementedError(
            f"dvcp: candidate grids above {ops.CPG_LDS_MAX_G}^3 are inference-only (G={int(G)}): the large-grid CPG "
            f"has no backward.  Run under torch.no_grad(), or train with int(2r/s + 1) <= {ops.CPG_LDS_MAX_G}")


def cpg(src, tgt, cand, G, cpg_module, large_grid=False):
    """cpg.py:27-60, differentiable in src, tgt and the conv weights: G <= 11 (dvcp_cpg_backward),
    and with ``large_grid=True`` G <= 32 (12..32: dvcp_cpg_tiled_backward)."""
    require_trainable_grid(G, large_grid)
    convs = [cpg_module.conv1, cpg_module.conv2, cpg_module.conv3]
    return _Cpg.apply(src, tgt, cand, G, *[t for c in convs for t in (c.weight, c.bias)])


def cpg1d(src, tgt, cand, cpg1d_module):
    """The paper's 1-D CPG (Sec. 3.6; dvcp_cpg1d / dvcp_cpg1d_backward), differentiable in src
    (B, K, 32), tgt (B, K, Gz, 32) and the three Conv1d layers of ``cpg1d_module`` (dvcp.paper.CPG1D)."""
    convs = [cpg1d_module.conv1, cpg1d_module.conv2, cpg1d_module.conv3]
    return _Cpg1d.apply(src, tgt, cand, *[t for c in convs for t in (c.weight, c.bias)])


def weighting(feat, weighting_module):
    """The paper's weighting layer (Sec. 3.2; dvcp_weighting / dvcp_weighting_backward) on rows
    (P, 32), differentiable in the rows and in ``weighting_module``'s (dvcp.paper.PaperWeighting)
    fc1-3 and bn1-2 weights and biases: the eval-mode BN is folded into the linear layers by torch ops
    recorded here (no cache), so torch carries the packed gradient back to them.  The running
    statistics get no gradient and are not updated."""
    return _Weighting.apply(feat, weighting_module.folded_params())


def weighting_bn(feat, weighting_module):
    """The paper's weighting layer in training mode (batch-statistics BN; dvcp/batchnorm.py
    ``weighting_train_forward`` / ``weighting_train_backward``, dvcp_weighting_bn_*) on rows (P, 32),
    differentiable in the rows and in fc1-3 and bn1-2's weights and biases.  The forward updates the
    running statistics once; a frozen parameter gets no gradient, but the layer still normalises with the
    batch's statistics."""
    m = weighting_module
    params = [t for lin, bn in ((m.fc1, m.bn1), (m.fc2, m.bn2)) for t in (lin.weight, lin.bias, bn.weight, bn.bias)]
    return _WeightingBN.apply(m, feat, *params, m.fc3.weight, m.fc3.bias)


def src_keypoints(fe_xyz, fe_feat, topk_idx, kstart, R_init, radius=1.0, nsample=32):
    """The key-point stage (deepVCP.py:39-68 + get_cat_feat_src.py), differentiable in fe_feat
    through the index_points gather (pointnet2_utils.py:59) and the distance weighting."""
    return _SrcKeypoints.apply(fe_xyz, fe_feat, topk_idx, kstart, R_init, radius, nsample)


def pose_loss(x, y_pred, R_true, t_true, alpha):
    """deepVCP_loss.py:105-121 on (B, 3, n) operands -> (loss, R, t); differentiable in y_pred."""
    return _PoseLoss.apply(x, y_pred, R_true, t_true, alpha)


# ---- paper mode: the extractor (dvcp.paper.PaperFeatExtraction) ------------------------------------

def _layer_grads(gp, chans, weight_shapes):
    """Packed per-layer dW | db | dgamma | dbeta -> [dW (as the conv's weight), db, dgamma, dbeta, ...]."""
    out, o = [], 0
    for (ci, co), shape in zip(zip(chans[:-1], chans[1:]), weight_shapes):
        out += [gp[o:o + co * ci].view(shape), gp[o + co * ci:o + co * ci + co],
                gp[o + co * ci + co:o + co * ci + 2 * co], gp[o + co * ci + 2 * co:o + co * ci + 3 * co]]
        o += co * ci + 3 * co
    return out


def _wanted(ctx, first, grads, dtypes):
    return [g.to(dt) if (g is not None and ctx.needs_input_grad[first + k]) else None
            for k, (g, dt) in enumerate(zip(grads, dtypes))]


def _fp_grads(ctx, gp, gp1, gp2, chans, nconv):
    """The tail of both propagation backwards: the packed gradient and the (B, N1, D1) / (B, N2, D2) rows
    as backward's return tuple."""
    per = _layer_grads(gp, chans, [ctx.shapes[4 * l][0] for l in range(nconv)] + [ctx.shapes[-2][0]])
    grads = per[:4 * nconv + (2 if len(chans) - 1 > nconv else 0)]   # a fused fc: its dgamma / dbeta are discarded
    gp1 = gp1.permute(0, 2, 1).to(ctx.in_dtypes[0]) if gp1 is not None else None
    gp2 = gp2.to(ctx.in_dtypes[1]) if gp2 is not None else None
    return (None, None, None, None, gp1, gp2, *_wanted(ctx, 6, grads, [dt for _, dt in ctx.shapes]))


def _sa_grads(ctx, gp, gF, chans):
    """The tail of both set-abstraction backwards, likewise."""
    grads = _layer_grads(gp, chans, [ctx.shapes[4 * l][0] for l in range(len(chans) - 1)])
    gF = gF.permute(0, 2, 1).to(ctx.feat_dtype) if gF is not None else None
    return (None, None, None, gF, None, None, None, *_wanted(ctx, 7, grads, [dt for _, dt in ctx.shapes]))


class _FeatureProp(torch.autograd.Function):
    """forward(fp, fc, xyz1, xyz2, p1, p2_rows, *[conv.weight, conv.bias, bn.weight, bn.bias per layer,
    then fc.weight, fc.bias]): saves the operands only; the backward recomputes the rest."""

    @staticmethod
    def forward(ctx, fp, fc, xyz1, xyz2, p1, p2_rows, *params):
        packed = fp.packed_params(fc)
        parts = []
        for bn in fp.mlp_bns:
            parts += [bn.running_mean.float(), torch.rsqrt(bn.running_var.double() + bn.eps).float()]
        if fc is not None:
            n = fc.weight.shape[0]
            parts += [torch.zeros(n, device=packed.device), torch.ones(n, device=packed.device)]
        p2 = p2_rows.detach()
        ctx.save_for_backward(xyz1, xyz2, p1, p2, packed, torch.cat(parts).contiguous())
        ctx.chans = fp.chans + ([fc.weight.shape[0]] if fc is not None else [])
        ctx.relu = [1] * len(fp.mlp_convs) + ([0] if fc is not None else [])
        ctx.nconv = len(fp.mlp_convs)
        ctx.shapes = [(p.shape, p.dtype) for p in params]
        ctx.in_dtypes = (None if p1 is None else p1.dtype, p2_rows.dtype)
        return ops.feature_propagation(xyz1, xyz2, p2, p1, ctx.chans, ctx.relu, packed)

    @staticmethod
    def backward(ctx, g):
        xyz1, xyz2, p1, p2, packed, bnstat = ctx.saved_tensors
        want_p1 = p1 is not None and ctx.needs_input_grad[4]
        want_p2 = ctx.needs_input_grad[5]
        gp, gp1, gp2 = ops.feature_propagation_backward(xyz1, xyz2, p2, p1, ctx.chans, ctx.relu, packed, bnstat, g,
                                                        want_p1=want_p1, want_p2=want_p2)
        return _fp_grads(ctx, gp, gp1, gp2, ctx.chans, ctx.nconv)


class _FeaturePropBN(torch.autograd.Function):
    """_FeatureProp with ``fp`` in training mode: batchnorm.fp_train_forward (statistics passes, running
    statistics updated, then the forward kernel) and fp_train_backward."""

    @staticmethod
    def forward(ctx, fp, fc, xyz1, xyz2, p1, p2_rows, *params):
        p2 = p2_rows.detach()
        out, st = batchnorm.fp_train_forward(fp, xyz1, xyz2, p1, p2, fc)
        ctx.save_for_backward(xyz1, xyz2, p1, p2, st["pack"], st["bnstat"])
        ctx.st = {k: st[k] for k in ("M", "chans", "relu", "nbn")}
        ctx.shapes = [(p.shape, p.dtype) for p in params]
        ctx.in_dtypes = (None if p1 is None else p1.dtype, p2_rows.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        xyz1, xyz2, p1, p2, pack, bnstat = ctx.saved_tensors
        st = dict(ctx.st, pack=pack, bnstat=bnstat)
        want_p1 = p1 is not None and ctx.needs_input_grad[4]
        want_p2 = ctx.needs_input_grad[5]
        gp, gp1, gp2 = batchnorm.fp_train_backward(st, xyz1, xyz2, p1, p2, g, want_p1=want_p1, want_p2=want_p2)
        return _fp_grads(ctx, gp, gp1, gp2, st["chans"], st["nbn"])


def _fp_tensors(fp, fc=None):
    out = []
    for conv, bn in zip(fp.mlp_convs, fp.mlp_bns):
        out += [conv.weight, conv.bias, bn.weight, bn.bias]
    return out + ([fc.weight, fc.bias] if fc is not None else [])


def feature_propagation(fp, xyz1, xyz2, p1, p2_rows, fc=None):
    """``fp.run`` (dvcp.paper.PointNetFeaturePropagation; dvcp_feature_propagation, the same kernel and
    bits) -> (B, N1, C) rows, differentiable in p1 (B, D1, N1), p2_rows (B, N2, D2), the layers' conv and
    BN weights and biases and the optional fused ``fc`` (backward: dvcp_feature_propagation_backward).
    The eval-mode BN is folded as for the SA layers: the packed dgamma / dbeta are bn.weight's /
    bn.bias' gradients, the running statistics are fixed.  With ``fp`` built with ``bn_train=True`` and in
    training mode: batch statistics (dvcp_feature_propagation_bn_stats / _bn_backward through
    dvcp/batchnorm.py), the running statistics updated once per call."""
    fn = _FeaturePropBN if (getattr(fp, "bn_train", False) and fp.training) else _FeatureProp
    return fn.apply(fp, fc, xyz1, xyz2, p1, p2_rows, *_fp_tensors(fp, fc))


class _GroupRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctr, xyz, feat, count, lst, nsample, radius):
        ctx.save_for_backward(count, lst)
        ctx.cfg = (int(nsample), feat.shape[1], feat.dtype)
        return ops.group_rows(ctr, xyz, feat.detach(), count, lst, nsample, radius)

    @staticmethod
    def backward(ctx, g):
        count, lst = ctx.saved_tensors
        ns, N, dtype = ctx.cfg
        gfeat = ops.group_rows_backward(count, lst, ns, N, g).to(dtype) if ctx.needs_input_grad[2] else None
        return None, None, gfeat, None, None, None, None


def group_rows(ctr, xyz, feat, count, lst, nsample, radius):
    """``ops.group_rows`` (ctr (B, Q, 3), xyz (B, 3, N), feat (B, N, 32)), differentiable in ``feat``
    (dvcp_group_rows_backward; the coordinate columns carry no gradient)."""
    return _GroupRows.apply(ctr, xyz, feat, count, lst, nsample, radius)


class _SaGroupMlp(torch.autograd.Function):
    """One set abstraction of the paper's extractor on fixed centres and lists: forward
    dvcp_sa_group_mlp, backward dvcp_sa_group_mlp_backward (eval-mode BN)."""

    @staticmethod
    def forward(ctx, sa, xyz, ctr, feat, count, lst, ns, *params):
        packed = sa.packed_params()
        ctx.save_for_backward(xyz, ctr, feat, count, lst, packed, _bn_stats(sa))
        ctx.chans, ctx.ns = list(sa.chans), int(ns)
        ctx.shapes = [(p.shape, p.dtype) for p in params]
        ctx.feat_dtype = None if feat is None else feat.dtype
        return ops.sa_group_mlp(xyz, ctr, feat, count, lst, ns, sa.chans, packed, xyz_pdim=2, feat_ddim=1, feat_pdim=2)

    @staticmethod
    def backward(ctx, g):
        xyz, ctr, feat, count, lst, packed, bnstat = ctx.saved_tensors
        want_feat = feat is not None and ctx.needs_input_grad[3]
        gp, gF = ops.sa_group_mlp_backward(xyz, ctr, feat, count, lst, ctx.ns, ctx.chans, packed, bnstat, g,
                                           want_feat_grad=want_feat)
        return _sa_grads(ctx, gp, gF, ctx.chans)


class _SaGroupMlpBN(torch.autograd.Function):
    """_SaGroupMlp with ``sa`` in training mode: batchnorm.train_forward (batch statistics, running
    statistics updated; the z rows kept when a backward will run) and train_backward."""

    @staticmethod
    def forward(ctx, sa, xyz, ctr, feat, count, lst, ns, *params):
        out, st = batchnorm.train_forward(sa, xyz, ctr, feat, count, lst, ns, keep_zrows=any(ctx.needs_input_grad))
        ctx.sa = sa
        ctx.lay = dict(pts=xyz, ctr=ctr, feat=feat, count=count, lst=lst, ns=int(ns), bn=st)
        ctx.shapes = [(p.shape, p.dtype) for p in params]
        ctx.feat_dtype = None if feat is None else feat.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        want_feat = ctx.lay["feat"] is not None and ctx.needs_input_grad[3]
        gp, gF = batchnorm.train_backward(ctx.sa, ctx.lay, g, want_feat_grad=want_feat)
        ctx.lay = None
        return _sa_grads(ctx, gp, gF, ctx.sa.chans)


def paper_feat_extraction(fe, pts, starts):
    """``PaperFeatExtraction.forward`` (pts (B, C, N), starts (3, B)) -> (B, N, 32), the same kernels and
    bits, differentiable in every parameter of ``fe``.  FPS and the ball queries run as in inference
    and carry no gradient; each set abstraction is paired with dvcp_sa_group_mlp_backward and each
    propagation with dvcp_feature_propagation_backward; torch adds a level's two consumers (f1: fp2's
    d p1 + sa2's feature gradient; f2: fp3's + sa3's).  Saved for backward: per level the coordinates,
    centres, counts, lists and feature rows.  The SA backward's feature scatter uses float atomics, so
    gradients upstream of it (sa1, sa2) are not bit-reproducible.  With ``fe`` built with ``bn_train=True``
    a module in training mode takes its batch-statistics pair instead (batchnorm.train_forward /
    train_backward for a set abstraction, fp_train_forward / fp_train_backward for a propagation)."""
    B, _, N = pts.shape
    xyz = pts[:, :3, :]
    feat = pts[:, 3:, :] if fe.use_normal else None
    levels = [(xyz, feat)]
    for sa, st in zip((fe.sa1, fe.sa2, fe.sa3), starts):
        pxyz, pf = levels[-1]
        with torch.no_grad():
            _, c = ops.fps(pxyz, sa.npoint, st.to(pts.device), pdim=2)
            ns = min(int(sa.nsample), pxyz.shape[2])
            count, lst, _ = ops.ball_query(pxyz, c, sa.radius, ns, pdim=2, cdim_pts=2)
        # each module follows its own .training (fe built with bn_train=True): batch statistics, or today's
        fn = _SaGroupMlpBN if (getattr(fe, "bn_train", False) and sa.training) else _SaGroupMlp
        rows = fn.apply(sa, pxyz, c, pf, count, lst, ns,
                                 *[t for conv, bn in zip(sa.mlp_convs, sa.mlp_bns)
                                   for t in (conv.weight, conv.bias, bn.weight, bn.bias)])
        levels.append((c, rows.permute(0, 2, 1)))
    (x0, f0), (x1, f1), (x2, f2), (x3, f3) = levels
    g2 = feature_propagation(fe.fp3, x2, x3, f2, f3.permute(0, 2, 1))
    g1 = feature_propagation(fe.fp2, x1, x2, f1, g2)
    return feature_propagation(fe.fp1, x0, x1, f0, g1, fc=fe.fc)


def _linears(m):
    return [m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, m.fc3.weight, m.fc3.bias]
