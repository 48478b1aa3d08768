"""Batch-statistics BatchNorm for the grouped set-abstraction MLP (training mode).

The reference trains the whole model in ``model.train()`` (train.py:105-125), so every
``F.relu(bn(conv(x)))`` of pointnet2_utils.py:195-200 normalises with the statistics of the current
batch over all B * S * nsample grouped entries (BatchNorm2d over (B, H, W); the padding slots of
the ball query are entries like any other) and updates the running statistics (momentum, unbiased
variance), once per FE1 call -- src and tgt are separate calls (deepVCP.py:29,72).

The REF-R tables with fp32 inputs (sa1 3[+3]-16-16-32, sa2, sa3) run on the matrix cores
(csrc/sa_bn_mfma.hip, ``_train_forward_mfma`` / ``_train_backward_mfma``): every pass recomputes
the MLP per 32-entry tile, nothing per entry is stored, and the weight gradients are MFMA products
over the entries.  The rest (fp64 inputs, channel-first feature tables) takes the lane-per-entry
passes below.

Forward (``train_forward``): one statistics pass per layer (dvcp_sa_bn_stats: fp64 sums of z and
z^2, the layers below normalised by their batch statistics), then the eval kernel
(dvcp_sa_group_mlp) with the batch statistics folded into its scale / shift.
Backward (``train_backward``): every entry's conv outputs z_l, written once by the forward's last
statistics pass (64-entry blocks, a few GB per call at C3 -- HBM is 288 GB -- held until the
backward; dvcp_sa_bn_zrows recomputes them when absent), then torch's batch-norm backward,
    dz_l = scale_l (dy_l - mean(dy_l) - xhat_l mean(dy_l xhat_l)),
whose mean terms make every entry's gradient non-zero: sums of the top layer over the routed
(arg-max) rows, one dense pass per lower layer for its sums, and a final dense pass for dW, db and
the per-entry rows of the weight gradients and the feature gradient (dvcp_sa_bn_backward modes
L..1, 0; csrc/sa_bn.hip); dW_l, db_l are then GEMMs over the entries (hipBLASLt via torch.bmm
over the rows' 65536-entry chunks, chunk sums in fp64).

Paper mode (dvcp/paper.py, ``bn_train=True``): the paper's sa1 table (3[+3]-32-32) takes the
lane-per-entry passes above; the feature propagations and the weighting layer have their own pairs at
the end of this file (``fp_train_forward`` / ``fp_train_backward``, csrc/paper_fe_bwd.hip's template
modes; ``weighting_train_forward`` / ``weighting_train_backward``, csrc/paper_wl_train.hip).
"""
import torch

from . import ops


def _layer_offsets(chans):
    """Per layer (offset, C_in, C_out) in the dvcp_sa_bn pack: W | bias | scale | shift | mean |
    istd | A/M | B/M."""
    offs, o = [], 0
    for cin, cout in zip(chans[:-1], chans[1:]):
        offs.append((o, cin, cout))
        o += cout * cin + 7 * cout
    return offs, o


def _update_running(bn, mean, var, M):
    """BatchNorm2d's running-statistics update in training mode (unbiased variance)."""
    if not bn.track_running_stats:
        return
    with torch.no_grad():
        bn.num_batches_tracked.add_(1)
        f = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
        unbiased = var * (M / max(M - 1, 1))
        bn.running_mean.mul_(1.0 - f).add_(mean.to(bn.running_mean.dtype), alpha=f)
        bn.running_var.mul_(1.0 - f).add_(unbiased.to(bn.running_var.dtype), alpha=f)


# z rows kept from the forward for the backward only up to this size per layer call (bytes); above
# it the backward recomputes them (dvcp_sa_bn_zrows), trading one pass for the memory.
ZROWS_KEEP_MAX_BYTES = 16 << 30


def _bnm_pack(sa, dev):
    offs, total = _layer_offsets(sa.chans)
    parts = []
    for conv, (o, cin, cout) in zip(sa.mlp_convs, offs):
        one, zero = torch.ones(cout, device=dev), torch.zeros(cout, device=dev)
        parts += [conv.weight.reshape(-1).float(), conv.bias.float(), one, zero, zero, one, zero, zero]
    pack = torch.cat(parts).contiguous()
    assert pack.numel() == total == ops.sa_bn_pack_floats(sa.chans)
    return pack, offs


def _batch_stats(bn, sums, M):
    """One BN layer's batch statistics from its fp64 sums (sum z | sum z^2 over the M values per
    channel): (mean, biased variance, rstd, scale, shift) in fp64, gamma and beta folded into scale |
    shift; and the running-statistics update."""
    mean = sums[0] / M
    var = (sums[1] / M - mean * mean).clamp_min(0.0)
    rstd = torch.rsqrt(var + bn.eps)
    scale = bn.weight.double() * rstd
    shift = bn.bias.double() - mean * scale
    _update_running(bn, mean, var, M)
    return mean, var, rstd, scale, shift


def _backward_sums(layers, sums_pass, out, M):
    """The backward's sums A = sum g_a | B = sum g_a xhat of every BN layer, the top layer first:
    ``layers`` lists (mode, offset, channels) top-down, ``sums_pass(mode)`` runs one layer's pass ->
    (2, C) fp64, which needs A/M | B/M of the layers above: written to ``out[offset:offset + 2 C]``
    before the next pass.  M = 0: zero sums, nothing written.  Returns {mode: sums}."""
    sums = {}
    for mode, off, c in layers:
        if M:
            sums[mode] = sums_pass(mode)
            out[off:off + 2 * c] = (sums[mode] / M).reshape(-1)
        else:
            sums[mode] = torch.zeros(2, c, dtype=torch.float64, device=out.device)
    return sums


def _set_stats(pack, bn, o, cin, cout, sums, M):
    """scale, shift, mean, istd of one layer into the dvcp_sa_bn pack."""
    mean, _, istd, scale, shift = _batch_stats(bn, sums, M)
    v = o + cout * cin + cout
    pack[v:v + 4 * cout] = torch.cat([scale, shift, mean, istd]).float()


def _train_forward_mfma(sa, xyz, ctr, feat, count, lst, ns):
    """The REF-R tables on the matrix cores (csrc/sa_bn_mfma.hip): (two-layer tables) the
    per-point half of layer 1 once, one statistics pass per layer, then the forward with its
    arg-max routing.  Nothing per entry is kept for the backward; it recomputes the MLP."""
    chans = sa.chans
    B, S = ctr.shape[0], ctr.shape[2]
    M = B * S * ns
    with torch.no_grad():
        pack, offs = _bnm_pack(sa, xyz.device)
        U = ops.sa_bnm_pre(feat, chans, pack) if len(chans) == 3 else None
        for layer, (bn, (o, cin, cout)) in enumerate(zip(sa.mlp_bns, offs), 1):
            sums = ops.sa_bnm_stats(xyz, ctr, feat, count, lst, ns, chans, pack, U, layer)
            _set_stats(pack, bn, o, cin, cout, sums, M)
        fwd = ops.sa_bnm_forward(xyz, ctr, feat, count, lst, ns, chans, pack, U)
    return fwd[0], dict(pack=pack, M=M, U=U, fwd=fwd, mfma=True)


def _train_backward_mfma(sa, lay, g_out, want_feat_grad):
    chans = sa.chans
    offs, _ = _layer_offsets(chans)
    st = lay["bn"]
    pack, M, U, fwd = st["pack"].clone(), st["M"], st["U"], st["fwd"]
    args = (lay["pts"], lay["ctr"], lay["feat"], lay["count"], lay["lst"], lay["ns"], chans)
    g = g_out.float().contiguous()
    out, _, zb = fwd
    L = len(offs)
    sums = [None] * L
    # the last layer's sums over the routed rows (gy = g at each (centre, channel)'s arg-max when
    # the max is positive): A = sum gy, B = sum gy xhat
    o, cin, cout = offs[-1]
    v = o + cout * cin
    mu, istd = pack[v + 3 * cout:v + 4 * cout], pack[v + 4 * cout:v + 5 * cout]
    gy = torch.where(out > 0, g, torch.zeros_like(g)).double()
    xh = ((zb - mu) * istd).double()
    sums[-1] = torch.stack([gy.sum((0, 1)), (gy * xh).sum((0, 1))])
    pack[v + 5 * cout:v + 7 * cout] = (sums[-1] / M).reshape(-1).float()
    for k in range(L - 1, 0, -1):   # each lower layer's sums need those of the layers above
        sums[k - 1] = ops.sa_bnm_backward(*args, pack, U, fwd, g, k)
        o, cin, cout = offs[k - 1]
        v = o + cout * cin
        pack[v + 5 * cout:v + 7 * cout] = (sums[k - 1] / M).reshape(-1).float()
    grads, gF = ops.sa_bnm_backward(*args, pack, U, fwd, g, 0, want_feat_grad=want_feat_grad)
    parts, i = [], 0
    for (o, cin, cout), s in zip(offs, sums):   # per layer dW, db, dgamma, dbeta
        parts += [grads[i:i + cout * cin + cout], s[1], s[0]]
        i += cout * cin + cout
    return torch.cat([p.float() for p in parts]), gF


# The matrix-core path for the tables it takes (tests switch it off to check the VALU passes).
USE_MFMA = True


def train_forward(sa, xyz, ctr, feat, count, lst, ns, keep_zrows=False):
    """pointnet2_utils.py:195-200 with ``sa`` in training mode, on (B, 3, N) points, (B, 3, S)
    centres and (B, D, N) features.  Returns (out (B, S, C_last) fp32, state for the backward).
    ``keep_zrows``: a backward will run (the autograd path), so the last statistics pass also
    writes every entry's z rows for it (within ZROWS_KEEP_MAX_BYTES); a train-mode forward with no
    backward (no_grad, frozen extractor) allocates none."""
    chans = sa.chans
    if USE_MFMA and ops.sa_bnm_usable(xyz, ctr, feat, chans):
        return _train_forward_mfma(sa, xyz, ctr, feat, count, lst, ns)
    dev = xyz.device
    B, S = ctr.shape[0], ctr.shape[2]
    M = B * S * ns
    with torch.no_grad():
        pack, offs = _bnm_pack(sa, dev)
        zrows = None
        keep = keep_zrows and ops.sa_bn_zrows_bytes(B, S, ns, chans) <= ZROWS_KEEP_MAX_BYTES
        for layer, (bn, (o, cin, cout)) in enumerate(zip(sa.mlp_bns, offs), 1):
            if keep and layer == len(offs):  # the last pass also writes every entry's z rows
                sums, zrows = ops.sa_bn_stats(xyz, ctr, feat, count, lst, ns, chans, pack, layer, want_zrows=True)
            else:
                sums = ops.sa_bn_stats(xyz, ctr, feat, count, lst, ns, chans, pack, layer)
            _set_stats(pack, bn, o, cin, cout, sums, M)
        fwd = torch.cat([pack[o:o + cout * cin + 3 * cout] for o, cin, cout in offs]).contiguous()
    out = ops.sa_group_mlp(xyz, ctr, feat, count, lst, ns, chans, fwd)
    return out, dict(pack=pack, M=M, zrows=zrows)


def train_backward(sa, lay, g_out, want_feat_grad):
    """Backward of ``train_forward``: (packed parameter gradient -- per layer dW, db, dgamma,
    dbeta -- and dL/d feat (B, N, D) fp32 or None)."""
    if lay["bn"].get("mfma"):
        return _train_backward_mfma(sa, lay, g_out, want_feat_grad)
    chans = sa.chans
    offs, _ = _layer_offsets(chans)
    st = lay["bn"]
    pack, M = st["pack"].clone(), st["M"]
    args = (lay["pts"], lay["ctr"], lay["feat"], lay["count"], lay["lst"], lay["ns"], chans)
    g = g_out.float().contiguous()
    # every entry's conv outputs with this batch's statistics: written by the forward's last
    # statistics pass (held from the forward to here), else recomputed now
    zrows = st.pop("zrows", None)
    if zrows is None:
        zrows = ops.sa_bn_zrows(*args, st["pack"])
    layers = [(k, o + cout * cin + 5 * cout, cout) for k, (o, cin, cout) in reversed(list(enumerate(offs, 1)))]
    sums = _backward_sums(layers, lambda k: ops.sa_bn_backward(*args, pack, zrows, g, k), pack, M)
    rows, gF = ops.sa_bn_backward(*args, pack, zrows, g, 0, want_feat_grad=want_feat_grad)
    del zrows
    parts = []
    for k, ((o, cin, cout), (gz, ha)) in enumerate(zip(offs, rows), 1):
        s = sums[k]
        dwb = _gemm_nt(gz, ha)                  # [dW | db] = dz [h; 1]^T over the M entries
        parts += [dwb[:, :cin].reshape(-1), dwb[:, cin], s[1], s[0]]   # dW, db, dgamma, dbeta
    return torch.cat([p.float() for p in parts]), gF


def _gemm_nt(a, b):
    """sum over chunks of a_k @ b_k^T for (nch, m, K) / (nch, n, K) chunked row tables: fp32 GEMMs
    (hipBLASLt via torch.bmm, B transposed by strides, no copy), the chunk products summed in fp64
    in a fixed order."""
    return torch.bmm(a, b.transpose(1, 2)).double().sum(0)


# ---- paper mode: feature propagation (dvcp.paper.PointNetFeaturePropagation, csrc/paper_fe_bwd.hip) ----
def fp_train_forward(fp, xyz1, xyz2, p1, p2_rows, fc=None):
    """``fp`` (Conv1d 1x1 + BN1d + ReLU per layer, optionally the fused ``fc`` as a plain last layer) in
    training mode: one statistics pass per BN layer (dvcp_feature_propagation_bn_stats, the layers below
    normalised by their batch statistics), mean / biased variance folded with gamma, beta into scale |
    shift in fp64 and rounded once, the running statistics updated, then the existing forward kernel on
    the finished pack: the train-mode forward adds no kernel.  Returns ((B, N1, C) rows, state for
    ``fp_train_backward``).  B N1 = 0: the rows are empty and nothing is updated."""
    B, N1 = xyz1.shape[0], xyz1.shape[2]
    M = B * N1
    require_batch(M, (B, fp.chans[0], N1))
    dev = xyz1.device
    chans = fp.chans + ([fc.weight.shape[0]] if fc is not None else [])
    relu = [1] * len(fp.mlp_convs) + ([0] if fc is not None else [])
    with torch.no_grad():
        parts, offs, o = [], [], 0
        for lin in list(fp.mlp_convs) + ([fc] if fc is not None else []):
            co, ci = lin.weight.shape[0], lin.weight.shape[1]
            parts += [lin.weight.reshape(-1).float(), lin.bias.float(), torch.ones(co, device=dev),
                      torch.zeros(co, device=dev)]
            offs.append((o, ci, co))
            o += ci * co + 3 * co
        pack = torch.cat(parts).contiguous()
        bnstat = torch.zeros(4 * sum(chans[1:]), dtype=torch.float64, device=dev)
        so = 0
        for layer, (o, ci, co) in enumerate(offs, 1):
            if layer > len(fp.mlp_bns):          # the fused fc: mean 0, rstd 1, no mean terms
                bnstat[so + co:so + 2 * co] = 1.0
            elif M:
                bn = fp.mlp_bns[layer - 1]
                sums = ops.feature_propagation_bn_stats(xyz1, xyz2, p2_rows, p1, chans, relu, pack, layer)
                mean, _, rstd, scale, shift = _batch_stats(bn, sums, M)
                v = o + co * ci + co
                pack[v:v + 2 * co] = torch.cat([scale, shift]).float()
                bnstat[so:so + 2 * co] = torch.cat([mean, rstd])
            so += 4 * co
        if M:
            out = ops.feature_propagation(xyz1, xyz2, p2_rows, p1, chans, relu, pack)
        else:
            out = torch.empty(B, N1, chans[-1], dtype=torch.float32, device=dev)
    return out, dict(pack=pack, bnstat=bnstat, M=M, chans=chans, relu=relu, nbn=len(fp.mlp_bns))


def fp_train_backward(st, xyz1, xyz2, p1, p2_rows, g, want_p1=True, want_p2=True):
    """Backward of ``fp_train_forward`` on its operands: (packed parameter gradient, per layer dW | db |
    dgamma | dbeta with dgamma = B and dbeta = A of the sums passes; d p1 (B, N1, D1) or None; d p2_rows
    (B, N2, D2) or None).  The top BN layer's sums first (dvcp_feature_propagation_bn_backward mode nbn),
    one pass per lower layer, then the gradient pass (mode 0)."""
    chans, relu, M = st["chans"], st["relu"], st["M"]
    bnstat = st["bnstat"].clone()
    args = (xyz1, xyz2, p2_rows, p1, chans, relu, st["pack"])
    layers = [(k, 4 * sum(chans[1:k]) + 2 * chans[k], chans[k]) for k in range(st["nbn"], 0, -1)]
    sums = _backward_sums(layers, lambda k: ops.feature_propagation_bn_backward(*args, bnstat, g, k), bnstat, M)
    gp, gp1, gp2 = ops.feature_propagation_bn_backward(*args, bnstat, g, 0, want_p1=want_p1, want_p2=want_p2)
    o = 0
    for k, (ci, co) in enumerate(zip(chans[:-1], chans[1:]), 1):
        if k in sums:
            gp[o + ci * co + co:o + ci * co + 3 * co] = torch.cat([sums[k][1], sums[k][0]]).float()
        o += ci * co + 3 * co
    return gp, gp1, gp2


# ---- paper mode: the weighting layer (dvcp.paper.PaperWeighting, csrc/paper_wl_train.hip) -------------
# (offset, C_in, C_out) of fc1 / fc2 in the train-mode pack W | b | scale | shift, then fc3, and the
# offset of each BN layer's mean | rstd | A/M | B/M in the statistics vector
_WL_LAYERS = ((0, 32, 16), (32 * 16 + 3 * 16, 16, 8))
_WL_STAT = (0, 4 * 16)


def require_batch(M, shape):
    """torch's refusal of batch statistics over a single value per channel."""
    if M == 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(shape)}")


def weighting_train_forward(wl, rows):
    """The paper's weighting layer (Sec. 3.2) with ``wl`` in training mode on rows (P, 32) fp32: one
    statistics pass per BN layer (dvcp_weighting_bn_stats: fp64 sums of z and z^2, the layer below
    normalised by its batch statistics), mean / biased variance folded into scale | shift in fp64 and
    rounded once, the running statistics updated (once per call), then the scores
    (dvcp_weighting_bn_forward).  Returns (scores (P,), state for ``weighting_train_backward``).  P = 0:
    no scores, no update."""
    P = rows.shape[0]
    require_batch(P, rows.shape)
    dev = rows.device
    with torch.no_grad():
        parts = []
        for lin in (wl.fc1, wl.fc2):
            c = lin.weight.shape[0]
            parts += [lin.weight.reshape(-1).float(), lin.bias.float(), torch.ones(c, device=dev),
                      torch.zeros(c, device=dev)]
        pack = torch.cat(parts + [wl.fc3.weight.reshape(-1).float(), wl.fc3.bias.float()]).contiguous()
        bnstat = torch.zeros(ops.WEIGHTING_BN_NSTAT, dtype=torch.float64, device=dev)
        if P == 0:
            return torch.empty(0, dtype=torch.float32, device=dev), dict(pack=pack, bnstat=bnstat, M=0, rows=rows)
        for layer, (bn, (o, cin, cout), so) in enumerate(zip((wl.bn1, wl.bn2), _WL_LAYERS, _WL_STAT), 1):
            mean, _, rstd, scale, shift = _batch_stats(bn, ops.weighting_bn_stats(rows, pack, layer), P)
            v = o + cout * cin + cout
            pack[v:v + 2 * cout] = torch.cat([scale, shift]).float()
            bnstat[so:so + 2 * cout] = torch.cat([mean, rstd])
        score = ops.weighting_bn_forward(rows, pack)
    return score, dict(pack=pack, bnstat=bnstat, M=P, rows=rows)


def weighting_train_backward(wl, st, g, want_feat):
    """Backward of ``weighting_train_forward``: ([d fc1.weight, d fc1.bias, d bn1.weight, d bn1.bias, d
    fc2.weight, d fc2.bias, d bn2.weight, d bn2.bias, d fc3.weight, d fc3.bias] fp32, d rows (P, 32) or
    None).  The top BN layer's sums first (dvcp_weighting_bn_backward mode 2), then the lower one's
    (mode 1), then the gradient pass (mode 0); d gamma = B and d beta = A are the sums themselves."""
    pack, M, rows = st["pack"], st["M"], st["rows"]
    bnstat = st["bnstat"].clone()
    layers = ((2, _WL_STAT[1] + 2 * 8, 8), (1, _WL_STAT[0] + 2 * 16, 16))
    sums = _backward_sums(layers, lambda mode: ops.weighting_bn_backward(rows, pack, bnstat, g, mode), bnstat, M)
    gp, gfeat = ops.weighting_bn_backward(rows, pack, bnstat, g, 0, want_feat=want_feat)
    w1, b1, w2, b2, w3, b3 = torch.split(gp, [16 * 32, 16, 8 * 16, 8, 8, 1])
    grads = [w1.view(16, 32), b1, sums[1][1].float(), sums[1][0].float(),
             w2.view(8, 16), b2, sums[2][1].float(), sums[2][0].float(), w3.view(1, 8), b3]
    return grads, gfeat
