"""The split-3 MFMA kernels (csrc/sa_mfma_*.hip, csrc/dfe_tgt.hip, csrc/cpg.hip; the split
itself in csrc/split3.h) may change their instruction stream -- how the split is written, what the
compiler may pack, where the VALU work sits between the MFMAs -- but never their arithmetic: the
same pieces, the same six products in the same order.  So

  * every output of tests/golden/mfma_stream.npz (recorded by tests/golden/make_mfma_stream.py
    before the stream was first touched) is reproduced bit for bit.  The fixture keeps an output as
    the SHA-256 of its bytes plus a sample of rows (the outputs are over the size a committed file
    may have; see the generator), so equal digests stand for torch.equal, and the sampled rows say
    where a difference sits;
  * for the target DFE, whose kernel is a software pipeline over the candidates of a wave
    (operands prepared one candidate ahead, rows gathered two ahead, kNN rows six ahead, unrolled
    by 8), permuting the candidates (cand, dist and idx rows together) permutes the output rows bit
    for bit: a pipeline slot fed another candidate's operands would show.  The same outputs are
    held to the oracle at test_dfe_tgt_fused_vs_oracle's tolerance.  These cases take standard
    normal features, as that test does; the fixture's cases take the generator's wide-range ones,
    for which an fp32 reference in another summation order is no yardstick.

The CPG's loop is unchanged (it takes split3.h's helpers as they were), so it has the fixture
cases only."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _gen():
    spec = importlib.util.spec_from_file_location("make_mfma_stream", os.path.join(GOLDEN, "make_mfma_stream.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _fixture():
    return np.load(os.path.join(GOLDEN, "mfma_stream.npz"))


def _check(name, out, ins):
    """`out` equals the fixture's record `name`; the inputs are checked first, so a changed
    random stream is reported as such."""
    M, z = _gen(), _fixture()
    got_in = np.stack([M.digest(t) for t in ins])
    assert np.array_equal(got_in, z[name + "::inputs"]), f"{name}: the seeded inputs differ from the recorded ones"
    rows = M.sample(out, int(z[name + "::step"]))
    want = z[name + "::rows"]
    bad = np.argwhere(rows.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (f"{name}: {len(bad)} sampled elements differ, first at {bad[0].tolist()}: "
                           f"{rows[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")
    assert np.array_equal(M.digest(out), z[name + "::sha256"]), f"{name}: differs outside the sampled rows"


@pytest.mark.parametrize("shape", ["flat", "xcd"])
@pytest.mark.parametrize("table", [0, 1, 2])
def test_sa_tables_equal_fixture(cuda, table, shape):
    M = _gen()
    c = M.sa_inputs(table, shape)
    ins = [c["xyz"], c["ctr"], c["count"], c["lst"]] + [c[k] for k in ("feat", "rows") if c[k] is not None]
    _check(f"sa{table + 1}_{shape}", M.sa_run(c, cuda), ins)


@pytest.mark.parametrize("case", range(5))
def test_dfe_tgt_equals_fixture(cuda, case):
    M = _gen()
    B, Mr, Q = M.DFE_CASES[case]
    ins = M.dfe_inputs(B, Mr, Q, wide_feat=True)
    for k, v in M.dfe_run(M.dfe_model(cuda), *ins, cuda).items():
        _check(f"dfe_{k}_B{B}_Q{Q}", v, list(ins))


@pytest.mark.parametrize("case", range(4))
def test_cpg_equals_fixture(cuda, case):
    M = _gen()
    B, K, r = M.CPG_CASES[case]
    src, tgt, cand, G = M.cpg_inputs(B, K, r)
    for k, v in M.cpg_run(M.cpg_model(cuda), src, tgt, cand, G, cuda).items():
        _check(f"cpg_{k}_B{B}_K{K}_G{G}", v, [src, tgt, cand])


@pytest.mark.parametrize("case", range(5))
def test_dfe_tgt_candidate_permutation_and_oracle(cuda, case):
    """Permuted candidates give permuted rows bit for bit (collapsed, literal and fp16-table
    kernels); the collapsed and literal outputs match the oracle's materialised
    Get_Cat_Feat_Tgt + feat_embedding_layer within rtol = atol = 1e-5."""
    import oracle as O
    from dvcp import ops
    M = _gen()
    B, Mr, Q = M.DFE_CASES[case]
    ref_xyz, feat, qry = M.dfe_inputs(B, Mr, Q, wide_feat=False, seed=7)
    torch.manual_seed(5)
    dfe_ref = O.feat_embedding_layer()
    mine = M.dfe_model(cuda)
    mine.load_state_dict(dfe_ref.state_dict())
    p = mine.packed_params()
    x, f, q = ref_xyz.to(cuda), feat.to(cuda), qry.to(cuda)
    dist, idx, _ = ops.knn(x, q, 32, ref_pdim=1, qry_pdim=1)
    perm = torch.randperm(Q, generator=torch.Generator().manual_seed(40 + case)).to(cuda)
    qp, dp, ip = q[:, perm].contiguous(), dist[:, perm].contiguous(), idx[:, perm].contiguous()
    outs = {}
    for name, ft, kw in (("collapsed", f, {}), ("literal", f, {"literal": True}), ("f16", f.half(), {})):
        got = ops.dfe_tgt(x, ft, q, dist, idx, p, ref_pdim=1, **kw)
        again = ops.dfe_tgt(x, ft, qp, dp, ip, p, ref_pdim=1, **kw)
        assert torch.equal(again, got[:, perm]), name
        outs[name] = got.cpu()
    with torch.no_grad():
        cat = O.Get_Cat_Feat_Tgt()(qry.view(B, Q, 1, 3), torch.zeros(B, Q, 3), ref_xyz, feat)
        want = dfe_ref(cat, src=False).view(B, Q, 32)
    for name in ("collapsed", "literal"):
        print(f"dfe_tgt {name} B={B} Q={Q}: max|err| {float((outs[name] - want).abs().max()):.2e}")
        torch.testing.assert_close(outs[name], want, rtol=1e-5, atol=1e-5)
