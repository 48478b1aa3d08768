"""Host check of the pose solve's 3x3 SVD (csrc/rigid_svd.h, host + device): a stand-alone
program built with the host compiler runs kabsch_svd on rank-deficient, tied and generic H with
U pre-poisoned (NaN), so a column the function leaves unwritten shows.  No GPU needed.

Checked against numpy fp64: R finite and orthogonal to 1e-12, tr(R H) >= sum sigma - 1e-12 sigma_1
(R = V U^T maximises tr(R H) over O(3)), det R = +1 where H is rank-deficient (U is completed to
det +1), R = I for H = 0, and R = V_np U_np^T to 1e-12 where sigma_3 / sigma_1 > 1e-6 (unique R).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG

PROGRAM = r"""
#include <cstdio>
#include <limits>
#include "rigid_svd.h"
int main() {
  double H[3][3];
  for (;;) {
    for (int i = 0; i < 9; ++i)
      if (std::scanf("%la", &H[i / 3][i % 3]) != 1) return 0;
    double R[3][3], U[3][3], sig[3];
    const double poison = std::numeric_limits<double>::quiet_NaN();
    for (int i = 0; i < 9; ++i) R[i / 3][i % 3] = U[i / 3][i % 3] = poison;
    dvcp::kabsch_svd(H, R, U, sig);
    for (int i = 0; i < 9; ++i) std::printf("%a ", R[i / 3][i % 3]);
    for (int i = 0; i < 9; ++i) std::printf("%a ", U[i / 3][i % 3]);
    std::printf("%a %a %a\n", sig[0], sig[1], sig[2]);
  }
}
"""


def _compiler():
    for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(c)
        if path:
            return path
    return None


@pytest.fixture(scope="module")
def kabsch_host(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("rigid_svd")
    src, exe = d / "main.cpp", d / "kabsch_host"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc"), str(src), "-o",
                    str(exe)], check=True)

    def run(Hs):
        Hs = np.asarray(Hs, np.float64).reshape(-1, 9)
        text = "\n".join(" ".join(float(v).hex() for v in row) for row in Hs) + "\n"
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout
        vals = np.array([[float.fromhex(v) for v in line.split()] for line in out.strip().splitlines()])
        assert vals.shape == (len(Hs), 21)
        return vals[:, :9].reshape(-1, 3, 3), vals[:, 9:18].reshape(-1, 3, 3), vals[:, 18:]

    return run


def _rot(g):
    q = np.linalg.qr(g.standard_normal((3, 3)))[0]
    return q * np.sign(np.linalg.det(q))


def _cases():
    g = np.random.default_rng(7)
    a, b = np.array([1.0, -2.0, 0.5]), np.array([0.25, 3.0, -1.0])
    P = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    Q1, Q2 = _rot(g), _rot(g)
    cop = Q1 @ np.diag([3.0, 1.5, 0.0]) @ Q2.T
    cases = {
        "zero": np.zeros((3, 3)),
        "rank1": np.outer(a, b),
        "rank1_axis": np.diag([1.0, 0.0, 0.0]),
        "rank1_last_axis": np.diag([0.0, 0.0, 2.0]),
        "rank1_small": 1e-100 * np.outer(a, b),   # squares stay above the sweep's 1e-300 absolute threshold
        "rank2": cop,
        "rank2_dyadic": np.array([[2.0, 1.0, 0.0], [0.5, 4.0, 0.0], [0.0, 0.0, 0.0]]),
        "equal3": 2.0 * np.eye(3),
        "equal3_perm": 2.0 * P,
        "equal3_reflect": 2.0 * np.diag([1.0, -1.0, 1.0]) @ P,
        "equal2": Q1 @ np.diag([3.0, 3.0, 1.0]) @ Q2.T,
        "near_equal": Q1 @ np.diag([3.0, 3.0 * (1 - 1e-9), 1.0]) @ Q2.T,
    }
    for k in range(6, 16):
        cases[f"rank2_eps1e-{k}"] = cop + 10.0 ** -k * np.outer(Q1[:, 2], Q2[:, 2])
    for i in range(8):
        cases[f"generic{i}"] = g.standard_normal((3, 3))
    return cases


def test_kabsch_svd_host(kabsch_host):
    cases = _cases()
    names = list(cases)
    H = np.stack([cases[k] for k in names])
    R, U, sig = kabsch_host(H)
    eye = np.eye(3)
    for k, name in enumerate(names):
        Un, s, Vt = np.linalg.svd(H[k])
        assert np.isfinite(R[k]).all() and np.isfinite(U[k]).all() and np.isfinite(sig[k]).all(), name
        assert np.abs(R[k].T @ R[k] - eye).max() <= 1e-12, (name, np.abs(R[k].T @ R[k] - eye).max())
        assert np.abs(U[k].T @ U[k] - eye).max() <= 1e-12, name
        assert np.trace(R[k] @ H[k]) >= s.sum() - 1e-12 * max(s[0], np.finfo(float).tiny), (name, np.trace(R[k] @ H[k]), s)
        assert np.abs(np.sort(sig[k])[::-1] - s).max() <= 1e-12 * max(s[0], np.finfo(float).tiny), (name, sig[k], s)
        if s[2] <= 1e-14 * s[0]:
            assert abs(np.linalg.det(U[k]) - 1.0) <= 1e-12 and abs(np.linalg.det(R[k]) - 1.0) <= 1e-12, name
        if s[0] > 0 and s[2] / s[0] > 1e-6:
            assert np.abs(R[k] - Vt.T @ Un.T).max() <= 1e-9, name     # the project's bar for R
    assert np.array_equal(R[names.index("zero")], eye)


def test_kabsch_svd_host_nan_stays_nan(kabsch_host):
    """A non-finite H (a weighted solve whose weights are all zero: 0 / 0 centroids) gives NaN, not
    a made-up rotation."""
    R, _, _ = kabsch_host(np.full((1, 3, 3), np.nan))
    assert np.isnan(R).all()
