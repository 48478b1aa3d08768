"""Paper-faithful mode (DeepVCP paper, Lu et al. ICCV 2019).  Not reference
parity: the reference repository implements a different network and none of
what follows runs in it.  Everything here is opt-in -- the reference path (dvcp.DeepVCP,
dvcp.deepVCP_loss) is untouched by it.  The checker is oracle/paper.py; DESIGN.md 4.6 lists the
choices the paper leaves open.

  * ``deepVCP_loss_paper`` / ``weighted_rigid_transform`` -- Sec. 3.4-3.5: weighted Kabsch with the
    key points' weights, reflection fix, the outlier rejection (the 20 % pairs with the largest
    residual under the first solve are dropped and the rest solved again) and the two-term L1
    loss.  Differentiable in the virtual corresponding points and the weights: the backward is
    HIP (dvcp_paper_pose_backward).
  * ``PointNetFeaturePropagation`` -- the reference's own dead layer (pointnet2_utils.py:265-315),
    one HIP kernel (dvcp_feature_propagation).
  * ``PaperFeatExtraction`` -- Sec. 3.1 + supplement: PointNet++ with three set-abstraction layers
    (4096 / 1024 / 256 samples) and three feature-propagation layers back to every input point,
    then a 32-unit fully connected layer (fused into the last propagation launch).
  * ``DeepVCPPaper`` -- the whole network with duplication (Sec. 3.6): a shared feature extractor
    and two cascaded stages, the second fed with the first's pose and generating candidates on a
    z line scored by a 1-D CNN (dvcp_cpg1d).  Inference by default; ``train_heads=True`` trains
    the two stages' heads (weighting layer, DFE, CPG) with the extractor frozen, and
    ``train_extractor=True`` the extractor with them (dvcp_feature_propagation_backward,
    dvcp_group_rows_backward, dvcp_sa_group_mlp_backward).  All of that with BatchNorm on its running
    statistics; ``bn_train=True`` makes ``.train()`` mean what it means in torch: every module with
    BatchNorm (the set abstractions, the propagations, ``PaperWeighting``) follows its own ``.training``
    and, in training mode, normalises with the batch's statistics and updates its running statistics
    (dvcp_sa_bn_*, dvcp_feature_propagation_bn_*, dvcp_weighting_bn_*; dvcp/batchnorm.py).
"""
import torch
import torch.nn as nn

from . import _lib, autograd, batchnorm, ops
from ._params import bn_affine, cached_pack
from .cpg import _wants_grad
from .cpg import cpg as _cpg3d
from .deep_feat_embedding import feat_embedding_layer
from .pointnet2_utils import PointNetSetAbstraction, _inference_only


def _b3n(t):
    return t.double().contiguous()


def weighted_rigid_transform(x, y, w=None, reflection_fix=True, inlier_ratio=1.0):
    """Weighted Kabsch on (B, 3, n) point sets (fp64): -> R (B, 3, 3), t (B, 3, 1).  ``w`` (B, n)
    weights (None = uniform; with reflection_fix=False, w=None and inlier_ratio=1 this is the
    reference's get_rigid_transform up to summation order); inlier_ratio < 1: the paper's
    rejection step."""
    return ops.paper_pose(x, y, w, reflection_fix=reflection_fix, inlier_ratio=inlier_ratio)


class _PaperLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, w, Rt, tt, alpha, reflection_fix, inlier_ratio):
        R, t, partial = ops.paper_pose(x, y, w, reflection_fix, inlier_ratio, Rt, tt)
        B, _, n = x.shape
        denom = float(B * 3 * n)
        loss = alpha * partial[:, 0].sum() / denom + (1 - alpha) * partial[:, 1].sum() / denom
        ctx.save_for_backward(x, y, w, Rt, tt)
        ctx.cfg = (alpha, reflection_fix, inlier_ratio)
        ctx.mark_non_differentiable(R, t)
        return loss, R, t

    @staticmethod
    def backward(ctx, g_loss, g_R, g_t):
        x, y, w, Rt, tt = ctx.saved_tensors
        alpha, refl, ratio = ctx.cfg
        gy, gw = ops.paper_pose_backward(x, y, w, Rt, tt, alpha, g_loss, refl, ratio, want_w=ctx.needs_input_grad[2])
        return None, gy, gw, None, None, None, None, None


def deepVCP_loss_paper(src_keypts, tgt_vcp, weights, R_true, t_true, alpha=0.5, reflection_fix=True,
                       inlier_ratio=1.0):
    """The paper's loss on key points x = src_keypts (B, K, 3), virtual corresponding points
    y* = tgt_vcp (B, K, 3) and key-point weights (B, K) (None = uniform): -> (loss, R, t).
    inlier_ratio = 0.8 is the paper's rejection step.  Differentiable in tgt_vcp and weights."""
    _lib.require_gpu(src_keypts, tgt_vcp, R_true, t_true)
    x = src_keypts.detach().permute(0, 2, 1).double().contiguous()
    y = tgt_vcp.permute(0, 2, 1).double()
    B, _, n = x.shape
    Rt = R_true.detach().double().expand(B, 3, 3).contiguous()
    tt = t_true.detach().double().reshape(-1, 3, 1).expand(B, 3, 1).contiguous()
    w = None if weights is None else weights.double().reshape(B, n)
    loss, R, t = _PaperLoss.apply(x, y.contiguous(), None if w is None else w.contiguous(), Rt, tt, float(alpha),
                                  bool(reflection_fix), float(inlier_ratio))
    return loss, R, t


# ------------------------------------------------------------------------------ feature extractor
class PointNetFeaturePropagation(nn.Module):
    """pointnet2_utils.py:265-315 (same parameters and state_dict keys: mlp_convs.i, mlp_bns.i);
    forward(xyz1 (B, 3, N), xyz2 (B, 3, S), points1 (B, D1, N) or None, points2 (B, D2, S)) ->
    (B, D', N), one HIP launch (eval-mode BN folded).  In eval mode with autograd on and a parameter or
    a feature input requiring a gradient, the output carries one (``autograd.feature_propagation``:
    the same forward kernel and bits, backward dvcp_feature_propagation_backward).

    ``bn_train`` (a plain attribute: no parameter or buffer).  False: training mode is refused.  True: in
    training mode every layer normalises with the batch mean and biased variance over the B N rows and
    updates running_mean / running_var / num_batches_tracked once per forward call (momentum, None
    included; unbiased variance): ``batchnorm.fp_train_forward`` (one dvcp_feature_propagation_bn_stats
    pass per layer, then the same forward kernel on the finished scale | shift), recorded by
    ``autograd.feature_propagation`` when something requires a gradient (backward:
    dvcp_feature_propagation_bn_backward), unrecorded otherwise, no_grad included.  B N = 1 raises
    ValueError before any launch, as torch does.  Eval mode: the paths above, bit for bit."""

    def __init__(self, in_channel, mlp, bn_train=False):
        super().__init__()
        self.bn_train = bool(bn_train)
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last = in_channel
        for out in mlp:
            self.mlp_convs.append(nn.Conv1d(last, out, 1))
            self.mlp_bns.append(nn.BatchNorm1d(out))
            last = out
        self.chans = [in_channel] + list(mlp)

    def packed_params(self, fc=None):
        """W | b | scale | shift per layer (BN folded), then the optional fc as a plain layer."""
        tensors = [t for conv, bn in zip(self.mlp_convs, self.mlp_bns)
                   for t in (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)]
        if fc is not None:
            tensors += [fc.weight, fc.bias]

        def build():
            parts = []
            for conv, bn in zip(self.mlp_convs, self.mlp_bns):
                scale, shift = bn_affine(bn)
                parts += [conv.weight.reshape(-1), conv.bias, scale, shift]
            if fc is not None:
                n = fc.weight.shape[0]
                parts += [fc.weight.reshape(-1), fc.bias, torch.ones(n, device=fc.weight.device),
                          torch.zeros(n, device=fc.weight.device)]
            return torch.cat(parts)

        return cached_pack(self, "fp" if fc is None else "fp_fc", tensors, build)

    def run(self, xyz1, xyz2, p1, p2_rows, fc=None):
        """-> (B, N, C) rows; p2_rows (B, S, D2) fp32 row-major, p1 (B, D1, N) view or None."""
        chans = self.chans + ([fc.weight.shape[0]] if fc is not None else [])
        relu = [1] * len(self.mlp_convs) + ([0] if fc is not None else [])
        return ops.feature_propagation(xyz1, xyz2, p2_rows, p1, chans, relu, self.packed_params(fc))

    def forward(self, xyz1, xyz2, points1, points2):
        p2_rows = points2.permute(0, 2, 1).contiguous().float()
        if self.bn_train and self.training:
            batchnorm.require_batch(xyz1.shape[0] * xyz1.shape[2], (xyz1.shape[0], self.chans[0], xyz1.shape[2]))
            _lib.require_gpu(xyz1, xyz2, points2)
            if _wants_grad(self, points2, *(() if points1 is None else (points1,))):
                return autograd.feature_propagation(self, xyz1, xyz2, points1, p2_rows).permute(0, 2, 1)
            return batchnorm.fp_train_forward(self, xyz1, xyz2, points1, p2_rows)[0].permute(0, 2, 1)
        _inference_only(self)
        if _wants_grad(self, points2, *(() if points1 is None else (points1,))):
            return autograd.feature_propagation(self, xyz1, xyz2, points1, p2_rows).permute(0, 2, 1)
        rows = self.run(xyz1, xyz2, points1, p2_rows)
        return rows.permute(0, 2, 1)


def paper_fe_config(use_normal=False, npoints=(4096, 1024, 256), radii=(0.1, 0.2, 0.4), nsample=32):
    """Supplement Sec. 1 (see oracle/paper.py)."""
    d0 = 3 if use_normal else 0
    sa = [dict(npoint=npoints[0], radius=radii[0], nsample=nsample, in_channel=3 + d0, mlp=[32, 32]),
          dict(npoint=npoints[1], radius=radii[1], nsample=nsample, in_channel=32 + 3, mlp=[32, 64]),
          dict(npoint=npoints[2], radius=radii[2], nsample=nsample, in_channel=64 + 3, mlp=[64, 64])]
    fp = [dict(in_channel=64 + 64, mlp=[64, 64]), dict(in_channel=32 + 64, mlp=[32, 32]),
          dict(in_channel=d0 + 32, mlp=[32, 32, 32])]
    return sa, fp


class PaperFeatExtraction(nn.Module):
    """Paper Sec. 3.1: per-point features (B, N, 32) for every input point.  forward(pts (B, C, N),
    starts=None (3, B) FPS starts, drawn like the reference's sample_and_group when None).  In eval mode
    with autograd on and a parameter (or ``pts``) requiring a gradient the features carry one
    (``autograd.paper_feat_extraction``: the same kernels and bits).  ``bn_train`` (a plain attribute,
    handed to the three propagations): False, ``.train()`` is refused; True, each set abstraction and each
    propagation follows its own ``.training`` (batch statistics and a running-statistics update per call
    in training mode, recorded or not), FPS and the ball queries as ever; two calls (source, then target)
    each use their own statistics.  The paper's dropout (keep 0.7) stays out, as in the checker."""

    def __init__(self, use_normal=False, bn_train=False, **cfg):
        super().__init__()
        self.use_normal = use_normal
        self.bn_train = bool(bn_train)
        sa, fp = paper_fe_config(use_normal, **cfg)
        self.sa1, self.sa2, self.sa3 = (PointNetSetAbstraction(**c) for c in sa)
        self.fp3, self.fp2, self.fp1 = (PointNetFeaturePropagation(bn_train=self.bn_train, **c) for c in fp)
        self.fc = nn.Linear(32, 32)

    def draw_starts(self, B, N):
        return torch.stack([torch.randint(0, n, (B,), dtype=torch.long)
                            for n in (N, self.sa1.npoint, self.sa2.npoint)])

    def _bn_modules(self):
        return (self.sa1, self.sa2, self.sa3, self.fp3, self.fp2, self.fp1)

    def forward(self, pts, starts=None):
        batch_stats = self.bn_train and (self.training or any(m.training for m in self._bn_modules()))
        if not batch_stats:
            _inference_only(self)
        B, _, N = pts.shape
        if starts is None:
            starts = self.draw_starts(B, N)
        if batch_stats:   # the composed path, recorded or not: each module on its own .training
            _lib.require_gpu(pts)
            return autograd.paper_feat_extraction(self, pts, starts)
        if _wants_grad(self, pts):
            return autograd.paper_feat_extraction(self, pts, starts)
        xyz = pts[:, :3, :]
        feat = pts[:, 3:, :] if self.use_normal else None
        levels = [(xyz, feat)]
        f_rows = None
        for sa, st in zip((self.sa1, self.sa2, self.sa3), starts):
            pxyz, pf = levels[-1]
            _, c = ops.fps(pxyz, sa.npoint, st.to(pts.device), pdim=2)
            ns = min(int(sa.nsample), pxyz.shape[2])
            count, lst, _ = ops.ball_query(pxyz, c, sa.radius, ns, pdim=2, cdim_pts=2)
            f_rows = ops.sa_group_mlp(pxyz, c, pf, count, lst, ns, sa.chans, sa.packed_params(), xyz_pdim=2,
                                      feat_ddim=1, feat_pdim=2)          # (B, S, C)
            levels.append((c, f_rows.permute(0, 2, 1)))
        (x0, f0), (x1, f1), (x2, f2), (x3, f3) = levels
        g2 = self.fp3.run(x2, x3, f2, f3.permute(0, 2, 1))                # (B, 1024, 64)
        g1 = self.fp2.run(x1, x2, f1, g2)                                 # (B, 4096, 32)
        return self.fp1.run(x0, x1, f0, g1, fc=self.fc)                   # (B, N, 32) incl. fc


class PaperWeighting(nn.Module):
    """Paper Sec. 3.2: FC 16 (BN, ReLU), FC 8 (BN, ReLU), FC 1 softplus; eval BN folded into the
    linear layers, one HIP launch (dvcp_weighting).  In eval mode with autograd on and a parameter or
    the input requiring a gradient, the scores carry one (backward: dvcp_weighting_backward, the fold
    differentiated by torch down to fc1-3 and bn1-2's weight / bias; running statistics are fixed).

    ``bn_train`` (a plain attribute: no parameter or buffer, the state_dict is the same either way).
    False: training mode is refused.  True: the module follows its own ``.training`` as torch's does.
    In training mode both BN layers normalise with the mean and biased variance of the call's B N rows
    and update running_mean / running_var / num_batches_tracked once per forward call (momentum, None
    included; unbiased variance): ``batchnorm.weighting_train_forward`` on its own entry points
    (dvcp_weighting_bn_stats / _forward / _backward, no fold), recorded by ``autograd.weighting_bn`` when
    something requires a gradient, run without recording otherwise (no_grad included: the running
    statistics are still updated).  A single row (B N = 1) raises ValueError before any launch, as
    torch does.  In eval mode the paths above, bit for bit.  The paper's dropout (keep 0.7) stays out:
    the checker has none in either mode."""

    def __init__(self, bn_train=False):
        super().__init__()
        self.bn_train = bool(bn_train)
        self.fc1, self.bn1 = nn.Linear(32, 16), nn.BatchNorm1d(16)
        self.fc2, self.bn2 = nn.Linear(16, 8), nn.BatchNorm1d(8)
        self.fc3 = nn.Linear(8, 1)

    def packed_params(self):
        tensors = [self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, self.fc3.weight, self.fc3.bias]
        tensors += [t for bn in (self.bn1, self.bn2) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)]

        return cached_pack(self, "pwl", tensors, self.folded_params)

    def folded_params(self):
        """W1 s1 | b1 s1 + h1 | W2 s2 | b2 s2 + h2 | W3 | b3 (s, h: the eval-mode BN as scale and shift),
        plain torch ops: differentiable in the parameters when autograd records them (the training
        path, uncached); ``packed_params`` caches the same values for inference."""
        parts = []
        for lin, bn in ((self.fc1, self.bn1), (self.fc2, self.bn2)):
            s, h = bn_affine(bn)
            parts += [(lin.weight * s[:, None]).reshape(-1), lin.bias * s + h]
        return torch.cat(parts + [self.fc3.weight.reshape(-1), self.fc3.bias])

    def forward(self, f):
        """(B, N, 32) -> (B, N) scores."""
        B, N, _ = f.shape
        if self.bn_train and self.training:
            batchnorm.require_batch(B * N, f.shape)
            _lib.require_gpu(f)
            if _wants_grad(self, f):
                return autograd.weighting_bn(f.reshape(B * N, 32), self).view(B, N)
            rows = f.detach().reshape(B * N, 32).contiguous().float()
            return batchnorm.weighting_train_forward(self, rows)[0].view(B, N)
        _inference_only(self)
        if _wants_grad(self, f):
            return autograd.weighting(f.reshape(B * N, 32), self).view(B, N)
        return ops.weighting(f.reshape(B * N, 32).contiguous().float(), self.packed_params()).view(B, N)


class CPG1D(nn.Module):
    """Paper Sec. 3.6: the back network's CPG, Conv1d 32-16-4-1 (k 3, p 1) over a z line of
    candidates, softmax, weighted candidate mean (one wave per key point, dvcp_cpg1d).  In eval mode
    with autograd on and a parameter or an input requiring a gradient, the output carries one
    (backward: dvcp_cpg1d_backward)."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv1d(32, 16, 3, padding=1)
        self.conv2 = nn.Conv1d(16, 4, 3, padding=1)
        self.conv3 = nn.Conv1d(4, 1, 3, padding=1)

    def packed_params(self):
        tensors = [t for c in (self.conv1, self.conv2, self.conv3) for t in (c.weight, c.bias)]
        return cached_pack(self, "cpg1d", tensors, lambda: torch.cat([t.reshape(-1) for t in tensors]))

    def forward(self, src, tgt, cand):
        _inference_only(self)
        if _wants_grad(self, src, tgt):
            return autograd.cpg1d(src, tgt, cand, self)
        return ops.cpg1d(src, tgt, cand, self.packed_params())


class _Stage(nn.Module):
    def __init__(self, one_d, bn_train=False):
        super().__init__()
        self.WL = PaperWeighting(bn_train=bn_train)
        self.DFE = feat_embedding_layer()
        self.cpg = CPG1D() if one_d else _cpg3d()
        self.one_d = one_d


def centred_grid(G, s, device, dtype=torch.float64):
    ax = (torch.arange(G, dtype=dtype, device=device) - (G - 1) / 2.0) * s
    return torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)


class DeepVCPPaper(nn.Module):
    """The paper's network with duplication (Sec. 3, 3.6; oracle/paper.py DeepVCPPaper is its
    checker; same submodule names and state_dict keys).  forward(src (B, C, N), tgt, R_init
    (B|1, 3, 3), t_init (B|1, 3[, 1])) -> list of per-stage dicts (keypts, vcp, weights, R, t, ...).
    ``starts``: (2, 3, B) FPS starts of the two FE calls; ``keypoint_idx``: optional per-stage
    (B, K) key-point overrides for stage-decoupled parity tests.

    ``train_heads`` (a plain attribute: no parameter or buffer, the state_dict is the same either
    way).  False: inference, whether or not autograd is on (nothing returned carries a gradient).
    True, in eval mode with autograd on: the two stages' heads train with the extractor frozen.
    FE and the full-cloud scores run under no_grad and give the top-k; the K selected rows' scores
    are recomputed differentiably (the layer is per row, so they are the gathered scores bit for
    bit, and the weighting backward runs on B K rows instead of B N); the source and target DFE rows
    go through ``autograd.dfe_rows``, the 3-D stage through ``autograd.cpg`` (the inference path's
    (B, K, 32, C) view; grids above 11^3 as ``autograd.require_trainable_grid`` rules) and the
    second stage through ``autograd.cpg1d``.  Stage 1's pose feeds stage 2 detached.  Each stage's
    ``vcp`` and ``weights`` carry a gradient; the caller sums ``deepVCP_loss_paper`` over the stages.
    A trainable FE parameter is refused (NotImplementedError) before any launch, and BatchNorm stays
    in eval mode (``.train()`` is refused as before).
    Memory: the materialised target rows (B, K C, 32, 35) fp32 are saved for backward: 4 * 32 * 35 *
    K * C bytes per pair, about 381 MB at K = 64, C = 1331 (computed, not measured); fusing them as the
    reference path's dvcp_dfe_tgt does is a later step.

    ``train_extractor`` (a plain attribute too).  True, in eval mode with autograd on: head training as
    above, and the extractor's trainable parameters train with it.  FE runs recorded for both clouds
    (``autograd.paper_feat_extraction``; the same parameters, so their gradients add); the full-cloud
    scores and the top-k stay under no_grad on the detached features; the K rows' scores are recomputed
    on the gathered, recorded features (dvcp_weighting_backward then returns d feat); the source and
    target rows go through ``autograd.group_rows`` and ``autograd.dfe_rows`` returns d rows (another
    4 * 32 * 35 * K * C bytes per pair on the target side while backward runs).  A frozen extractor
    under ``train_extractor=True`` is head training, bit for bit.  With the switch off nothing changes,
    the refusal under ``train_heads=True`` included.

    ``bn_train`` (a plain attribute too, handed to ``FE`` and to both stages' ``PaperWeighting``).  False:
    ``.train()`` is refused as before.  True: every module follows its own ``.training``, so
    ``model.train()`` trains with batch statistics throughout and ``model.train(); model.FE.eval()`` is
    frozen-BN fine-tuning of the extractor under batch-statistics heads.  ``FE`` runs once per cloud (source,
    then target), each call with its own statistics and its own running update.  A stage whose ``WL`` is
    in training mode calls it once on all B N source rows (statistics over B N, running statistics
    updated once per stage and forward; recorded when training, unrecorded otherwise); the top-k runs
    on the detached scores and ``weights`` is a gather of the recorded scores, so d loss / d weights
    reaches every row through the BN backward.  It is never called again on the K gathered rows (other
    statistics, a second update).  With ``WL`` in eval mode the K-row recomputation above is unchanged.
    ``train_heads`` / ``train_extractor`` keep their meaning: they decide what is recorded, ``.training``
    which statistics.  DFE, the 3-D CPG and the 1-D CPG have no BatchNorm.  The paper's dropout (keep
    0.7) stays out: the checker has none in either mode."""

    def __init__(self, use_normal=False, K=64, r=2.0, s=0.4, s_z=0.25, d=1.0, nsample=32, duplication=True,
                 inlier_ratio=0.8, train_heads=False, train_extractor=False, bn_train=False, **fe_cfg):
        super().__init__()
        self.train_heads = bool(train_heads)
        self.train_extractor = bool(train_extractor)
        self.bn_train = bool(bn_train)
        self.FE = PaperFeatExtraction(use_normal, bn_train=self.bn_train, **fe_cfg)
        self.stages = nn.ModuleList([_Stage(one_d, self.bn_train) for one_d in ((False, True) if duplication
                                                                                 else (False,))])
        self.K, self.r, self.s, self.s_z, self.d, self.ns = K, r, s, s_z, d, nsample
        self.inlier_ratio = inlier_ratio

    def forward(self, src, tgt, R_init, t_init, starts=None, keypoint_idx=None):
        if not self.bn_train:
            _inference_only(self)
        train = (self.train_heads or self.train_extractor) and torch.is_grad_enabled()
        if train:
            if not self.train_extractor and any(p.requires_grad for p in self.FE.parameters()):
                raise NotImplementedError("dvcp: DeepVCPPaper(train_heads=True) trains the stage heads only: the "
                                          "extractor must be frozen (model.FE.requires_grad_(False))")
            autograd.require_trainable_grid(int(2 * self.r / self.s + 1), self.stages[0].cpg.train_large_grid)
        _lib.require_gpu(src, tgt)
        with torch.enable_grad() if train else torch.no_grad():
            return self._stages(src, tgt, R_init, t_init, starts, keypoint_idx, train)

    def _stages(self, src, tgt, R_init, t_init, starts, keypoint_idx, train):
        B, _, N = src.shape
        dev = src.device
        if starts is None:
            starts = torch.stack([self.FE.draw_starts(B, N), self.FE.draw_starts(B, tgt.shape[2])])
        with torch.enable_grad() if (train and self.train_extractor) else torch.no_grad():
            f_src, f_tgt = self.FE(src, starts[0]), self.FE(tgt, starts[1])   # recorded: trainable FE parameters
        rows_of = lambda f: autograd.group_rows if f.requires_grad else ops.group_rows   # noqa: E731
        xs, xt = src[:, :3, :], tgt[:, :3, :]
        xs_rows = xs.permute(0, 2, 1)
        Rc = R_init.to(dev, torch.float64).expand(B, 3, 3)
        tc = t_init.to(dev, torch.float64).reshape(-1, 3).expand(B, 3)
        out = []
        for si, st in enumerate(self.stages):
            wl_bn = st.WL.bn_train and st.WL.training
            if wl_bn:   # batch statistics over all B N rows: one call, recorded when training
                recorded = st.WL(f_src)
                score = recorded.detach()
            else:
                with torch.no_grad():
                    score = st.WL(f_src.detach())
            top = ops.topk(score, self.K) if keypoint_idx is None else keypoint_idx[si].to(dev, torch.int64)
            if wl_bn:   # never a second call on the K rows: other statistics, a second running update
                w = torch.gather(recorded, 1, top)
            elif train:   # the K selected rows again, recorded: the gathered scores bit for bit
                w = st.WL(torch.gather(f_src, 1, top[..., None].expand(B, self.K, 32)))
            else:
                w = torch.gather(score, 1, top)
            kp = torch.gather(xs_rows, 1, top[..., None].expand(B, self.K, 3)).contiguous()   # (B, K, 3)
            ns_src = min(self.ns, N)
            cnt, lst, _ = ops.ball_query(xs, kp, self.d, ns_src, pdim=2, cdim_pts=1)
            rows = rows_of(f_src)(kp, xs, f_src, cnt, lst, self.ns, self.d)
            dfe = (lambda X: autograd.dfe_rows(X, st.DFE)) if train else (lambda X: ops.dfe(X, st.DFE.packed_params()))
            src_dfe = dfe(rows)                                                              # (B, K, 32)
            moved = torch.einsum("bij,bkj->bki", Rc, kp.double()) + tc[:, None, :]
            if st.one_d:
                G = int(2 * self.r / self.s_z + 1)
                off = torch.zeros(G, 3, dtype=torch.float64, device=dev)
                off[:, 2] = (torch.arange(G, dtype=torch.float64, device=dev) - (G - 1) / 2.0) * self.s_z
            else:
                G = int(2 * self.r / self.s + 1)
                off = centred_grid(G, self.s, dev)
            cand = (moved[:, :, None, :] + off[None, None]).float().contiguous()            # (B, K, C, 3)
            C = cand.shape[2]
            qry = cand.view(B, self.K * C, 3)
            ns_tgt = min(self.ns, xt.shape[2])
            cnt, lst, _ = ops.ball_query(xt, qry, self.d, ns_tgt, pdim=2, cdim_pts=1)
            trows = rows_of(f_tgt)(qry, xt, f_tgt, cnt, lst, self.ns, self.d)
            tgt_dfe = dfe(trows).view(B, self.K, C, 32)    # train: trows (B, K C, 32, 35) saved for backward
            # 3-D: cpg.py:34's reshape of a (B, K, 32, C) view whose row-major order is the
            # candidates' own: the 3-D grid without the reference's Q11 scramble
            if st.one_d:
                vcp = (autograd.cpg1d(src_dfe, tgt_dfe, cand, st.cpg) if train
                       else ops.cpg1d(src_dfe, tgt_dfe, cand, st.cpg.packed_params()))
            elif train:
                vcp = autograd.cpg(src_dfe, tgt_dfe.contiguous().view(B, self.K, 32, C), cand, G, st.cpg,
                                   large_grid=st.cpg.train_large_grid)
            else:
                vcp = ops.cpg(src_dfe, tgt_dfe.contiguous().view(B, self.K, 32, C), cand, G,
                              st.cpg.packed_params())
            # the pose carries no gradient (stage 2 starts from it detached, as the checker's numpy solve)
            R, t = ops.paper_pose(kp.permute(0, 2, 1), vcp.detach().permute(0, 2, 1), w.detach(), True,
                                  self.inlier_ratio)
            Rc, tc = R, t.reshape(B, 3)
            out.append(dict(keypts=kp, vcp=vcp, weights=w, R=R, t=t, topk=top, cand=cand, src_dfe=src_dfe,
                            tgt_dfe=tgt_dfe, score=score))
        return out


__all__ = ["deepVCP_loss_paper", "weighted_rigid_transform", "PointNetFeaturePropagation", "PaperFeatExtraction",
           "PaperWeighting", "CPG1D", "DeepVCPPaper", "paper_fe_config"]
