"""Host side of the direct transform (no GPU): the Gaussian quadrature weights at the grid's own latitudes, the C ABI of the new
entry points, and the resources of its two kernels."""
import os
import re
import sys

import numpy as np
import pytest

import atlas_amd
from atlas_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exact_weights(N):
    """Gauss-Legendre weights of 2N points, north to south: numpy's nodes polished by Newton steps and the weights evaluated in
    long double.  (numpy's own leggauss weights carry errors that grow with N: 5e-11 at N = 160 and 1.4e-7 at N = 1280 near the
    poles, measured against a 50-digit evaluation; its nodes are accurate.)"""
    x, _ = np.polynomial.legendre.leggauss(2 * N)
    x = x[::-1].astype(np.longdouble)
    n = 2 * N

    def p_and_d(x):
        p0, p1 = np.ones_like(x), x.copy()
        for k in range(2, n + 1):
            p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
        return p1, n * (p0 - x * p1)          # P_n, (1 - x^2) P'_n
    for _ in range(2):
        p, d = p_and_d(x)
        x = x - p * (1 - x * x) / d
    _, d = p_and_d(x)
    return np.asarray(2 * (1 - x * x) / (d * d), dtype=np.float64)


@pytest.mark.parametrize("N", [16, 32, 80, 160, 640, 1280])
def test_gaussian_weights(N):
    g = atlas_amd.Grid(f"O{N}")
    w = g.gaussian_weights()
    ref = exact_weights(N)
    rel = np.max(np.abs(w - ref) / ref)
    # the grid's latitudes are the reference's tables, printed with 12 decimals (16 for N16 / N24): the weights at
    # those latitudes differ from the exact ones by up to 2.3e-13 (N = 160), 1.2e-10 (N = 1280, the polar row) -- observed here
    tol = 1e-12 if N <= 160 else 2e-10
    assert rel <= tol, (N, rel)
    lg = np.polynomial.legendre.leggauss(2 * N)[1][::-1]   # numpy's weights: within their own accuracy
    assert np.max(np.abs(w - lg) / lg) <= (1e-10 if N <= 160 else 1e-6)
    assert abs(w.sum() - 2.0) <= 1e-14
    assert np.array_equal(w, w[::-1])
    assert np.array_equal(atlas_amd.Grid(f"F{N}").gaussian_weights(), w)


def test_gaussian_weights_of_a_classic_grid_and_refusal_of_others():
    w = atlas_amd.Grid("N32").gaussian_weights()
    assert w.shape == (64,) and abs(w.sum() - 2.0) <= 1e-14
    g = atlas_amd.StructuredGrid(nx=np.full(8, 16), y=np.linspace(70.0, -70.0, 8))
    with pytest.raises(_lib.AtlasAmdError, match="not a global Gaussian grid"):
        g.gaussian_weights()


def test_new_entry_points_are_declared_and_refuse_a_null_handle():
    text = open(os.path.join(ROOT, "include", "atlas_amd.h")).read()
    for name in ("atlas_amd__Trans__dirtrans_scalar_device", "atlas_amd__Trans__timings_dirtrans", "atlas_amd__Grid__gaussian_weights"):
        assert re.search(r"\b" + name + r"\s*\(", text), name
    assert _lib.Trans_dirtrans_scalar_device(None, 1, None, None) != 0
    assert _lib.last_error().decode().startswith("Not implemented: dirtrans")
    assert _lib.Trans_dirtrans_field(None, None, None) != 0
    assert _lib.last_error().decode().startswith("Not implemented")
    assert _lib.Grid_gaussian_weights(None, None) != 0


sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402


@pytest.mark.skipif(not os.path.exists(os.path.join(kr.LLVM, "llvm-readelf")), reason="llvm-readelf of the ROCm toolchain not found")
def test_dirtrans_kernels_have_no_spills_and_no_scratch(lib_built):
    ks = {kr.short(k["demangled"]): k for k in kr.kernels()}
    names = [n for n in ks if re.search(r"trans::(fft_fwd_rows_kernel|legendre_dir_kernel<[246]>)$", n)]
    assert len(names) == 4, names
    bad = [(n, ks[n]["vgpr_spill_count"], ks[n]["scratch"]) for n in names
           if ks[n]["vgpr_spill_count"] or ks[n]["scratch"] or ks[n]["dynamic_stack"]]
    assert not bad, bad
