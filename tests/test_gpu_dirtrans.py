"""Direct transform of scalar fields (Trans(grid, T, dirtrans=1)): round trips through invtrans, an independent numpy restatement
(np.fft.rfft per row, the oracle's Fourier truncation cut-off and Legendre functions, Gaussian weights), bitwise invariances, and
what is refused."""
import numpy as np
import pytest

import atlas_amd
import oracle
from atlas_amd import _lib
from helpers import red_spectra

pytestmark = pytest.mark.gpu


def pos(T, m, n):
    return (2 * T + 3 - m) * m // 2 + n - m


def spectra_without_last_column(T, nf, seed):
    """random spectra (TransLocal layout) whose m = T column is zero: the scalar invtrans drops m = T"""
    sp = red_spectra(T, nf, seed=seed).reshape(-1, 2, nf)
    sp[pos(T, T, T)] = 0.0
    return sp.reshape(-1)


def gauss_weights(N, lat_deg):
    """w = 2 / ((1 - x^2) P'_2N(x)^2) in numpy long double at the given latitudes"""
    x = np.sin(np.deg2rad(np.asarray(lat_deg, dtype=np.longdouble)))
    n = 2 * N
    p0, p1 = np.ones_like(x), x.copy()
    for k in range(2, n + 1):
        p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
    d = n * (p0 - x * p1)
    return np.asarray(2 * (1 - x * x) / (d * d), dtype=np.float64)


def restatement(g, T, gp, fields, ms=None):
    """a[m][n] for the given fields (list of field indices into gp reshaped (nf, npts)): rfft per row / n_j, kept m <= M_j (the
    inverse's cut-off, from the oracle's nlat0), a = 1/2 sum_j w_j P_n^m(mu_j) F_m(j).  Returns {f: array (T+1)(T+2) layout [pos][2]}"""
    nx, lat = g.nx(), g.y()
    ny = len(nx)
    plan = oracle.OraclePlan(T, nx, lat, with_tables=False)
    nlat0 = plan.nlat0
    ms = list(range(T + 1)) if ms is None else list(ms)
    w = gauss_weights(ny // 2, lat)
    rowoff = np.concatenate([[0], np.cumsum(nx)])
    out = {f: np.zeros(((T + 1) * (T + 2) // 2, 2)) for f in fields}
    acc = {f: {m: np.zeros(T + 1 - m, dtype=complex) for m in ms} for f in fields}
    for jleg in range((ny + 1) // 2):
        mj = [m for m in ms if nlat0[m] <= jleg]
        if not mj:
            continue
        lp = oracle.legendre_lat(T, np.deg2rad(lat[jleg]))
        for j in sorted({jleg, ny - 1 - jleg}):
            for f in fields:
                row = gp[f][rowoff[j]:rowoff[j + 1]]
                X = np.fft.rfft(row) / nx[j]
                for m in mj:
                    P = lp[pos(T, m, m):pos(T, m, T) + 1]
                    if j != jleg:   # southern row: P_n^m(-mu) = (-1)^(n-m) P_n^m(mu)
                        P = P * (-1.0) ** np.arange(T + 1 - m)
                    acc[f][m] += 0.5 * w[j] * P * X[m]
    for f in fields:
        for m in ms:
            k0 = pos(T, m, m)
            out[f][k0:k0 + T + 1 - m, 0] = acc[f][m].real
            out[f][k0:k0 + T + 1 - m, 1] = acc[f][m].imag if m > 0 else 0.0
    return out, nlat0


def field_of(sp, T, nf, f):
    return sp.reshape(-1, 2, nf)[:, :, f]


@pytest.mark.parametrize("grid,T", [("F16", 31), ("F32", 63), ("F80", 159), ("F32", 42), ("F32", 31)])
def test_round_trip_on_full_gaussian_grids(grid, T):
    """dirtrans(invtrans(s)) = s where quadrature and rows are exact (T < 2N, full rows): linear, quadratic and cubic T"""
    g = atlas_amd.Grid(grid)
    nf = 3
    tr = atlas_amd.Trans(g, T, dirtrans=1)
    sp = spectra_without_last_column(T, nf, seed=T)
    gp = np.zeros(nf * g.size())
    tr.invtrans(nf, sp, gp)
    back = np.full_like(sp, np.nan)
    tr.dirtrans(nf, gp, back)
    err = np.max(np.abs(back - sp)) / np.max(np.abs(sp))
    assert err <= 1e-12, (grid, T, err)


@pytest.mark.parametrize("grid,T", [("O32", 31), ("O80", 159), ("N32", 31)])
def test_reduced_grids_against_numpy_restatement(grid, T):
    g = atlas_amd.Grid(grid)
    nf = 2
    tr = atlas_amd.Trans(g, T, dirtrans=1)
    rng = np.random.default_rng(7)
    gp = rng.standard_normal(nf * g.size())
    sp = np.full(nf * tr.nb_spectral_coefficients(), np.nan)
    tr.dirtrans(nf, gp, sp)
    ref, nlat0 = restatement(g, T, gp.reshape(nf, -1), range(nf))
    # rows with M_j < T exist: the cut-off matters (the polar rows of a reduced grid keep fewer wavenumbers)
    assert nlat0.max() > 0
    for f in range(nf):
        a = field_of(sp, T, nf, f)
        err = np.max(np.abs(a - ref[f])) / np.max(np.abs(ref[f]))
        assert err <= 1e-12, (grid, f, err)
        assert np.all(a[pos(T, 0, 0):pos(T, 0, T) + 1, 1] == 0.0)   # Im a_n^0 exactly 0


def test_tl1279_o1280_137_fields():
    """headline size: TL1279 -> O1280, 137 fields; wavenumbers {0, 1, 2, 319, 640, 1000, 1278, 1279} of fields {0, 68, 136} against
    the restatement (observed on MI355X: see DESIGN 3.6), and a field of the 137-field call equals a 1-field call bitwise"""
    import torch
    g = atlas_amd.Grid("O1280")
    T, nf = 1279, 137
    tr = atlas_amd.Trans(g, T, dirtrans=1)
    npts = g.size()
    ncoef = tr.nb_spectral_coefficients()
    gen = torch.Generator(device="cuda").manual_seed(1279)
    gp = torch.randn(nf * npts, dtype=torch.float64, device="cuda", generator=gen)
    sp = torch.full((nf * ncoef,), float("nan"), dtype=torch.float64, device="cuda")
    tr.dirtrans(nf, gp, sp)
    torch.cuda.synchronize()
    fields = [0, 68, 136]
    sp_h = sp.view(-1, 2, nf)[:, :, fields].cpu().numpy()
    assert np.isfinite(sp_h).all()
    gp_h = {f: gp[f * npts:(f + 1) * npts].cpu().numpy() for f in fields}
    ms = [0, 1, 2, 319, 640, 1000, 1278, 1279]
    ref, _ = restatement(g, T, gp_h, fields, ms=ms)
    worst = 0.0
    for i, f in enumerate(fields):
        for m in ms:
            k0, k1 = pos(T, m, m), pos(T, m, T) + 1
            a, r = sp_h[k0:k1, :, i], ref[f][k0:k1]
            scale = max(np.max(np.abs(r)), 1e-300)
            worst = max(worst, np.max(np.abs(a - r)) / scale)
    print(f"TL1279 -> O1280: max |a - restatement| / max |a| per (field, m) = {worst:.2e}")
    assert worst <= 1e-10, worst
    for f in fields:   # the 1-field call of field f: bitwise the same
        one = torch.full((ncoef,), float("nan"), dtype=torch.float64, device="cuda")
        tr.dirtrans(1, gp[f * npts:(f + 1) * npts].contiguous(), one)
        torch.cuda.synchronize()
        assert torch.equal(one.view(-1, 2), sp.view(-1, 2, nf)[:, :, f]), f


def test_entry_points_agree_bitwise_and_a_graph_replay_equals_the_direct_call():
    import torch
    g = atlas_amd.Grid("O48")
    T, nf = 47, 5
    tr = atlas_amd.Trans(g, T, dirtrans=1, profile=1)
    npts, ncoef = g.size(), tr.nb_spectral_coefficients()
    rng = np.random.default_rng(11)
    gp = rng.standard_normal(nf * npts)
    host = np.full(nf * ncoef, np.nan)
    tr.dirtrans(nf, gp, host)
    # device (torch)
    gp_d = torch.from_numpy(gp).cuda()
    sp_d = torch.full((nf * ncoef,), float("nan"), dtype=torch.float64, device="cuda")
    tr.dirtrans(nf, gp_d, sp_d)
    torch.cuda.synchronize()
    assert np.array_equal(sp_d.cpu().numpy(), host)
    # Field / FieldSet: one field each, layout [pos][2]
    gps = [np.ascontiguousarray(gp[f * npts:(f + 1) * npts]) for f in range(nf)]
    sps = [np.full(ncoef, np.nan) for _ in range(nf)]
    tr.dirtrans_fieldset(gps, sps)
    one = np.full(ncoef, np.nan)
    tr.dirtrans_field(gps[2], one)
    for f in range(nf):
        assert np.array_equal(sps[f], host.reshape(-1, nf)[:, f]), f
    assert np.array_equal(one, sps[2])
    t = tr.timings_dirtrans(reset=True)
    assert t["fourier_calls"] >= 2 and t["legendre_calls"] == t["fourier_calls"] and t["legendre_ms"] > 0 and t["fourier_ms"] > 0
    # HIP graph: after the first call of the shape the device entry point only launches kernels on the object's stream
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        tr.set_profile(False)
        tr.use_torch_stream()
        tr.dirtrans(nf, gp_d, sp_d)
        side.synchronize()
        ref = sp_d.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            tr.dirtrans(nf, gp_d, sp_d)
        for _ in range(2):
            sp_d.fill_(float("nan"))
            graph.replay()
            side.synchronize()
            assert torch.equal(sp_d, ref)
    assert np.array_equal(ref.cpu().numpy(), host)


def test_default_objects_refuse_with_the_hint():
    g = atlas_amd.Grid("O32")
    tr = atlas_amd.Trans(g, 31)
    for call in (lambda: tr.dirtrans(1, None, None), lambda: tr.dirtrans_field(None, None),
                 lambda: tr.dirtrans_fieldset([], [])):
        with pytest.raises(NotImplementedError, match=r"^Not implemented.*dirtrans=1"):
            call()
    tr1 = atlas_amd.Trans(g, 31, dirtrans=1)
    for call in (lambda: tr1.dirtrans_wind2vordiv(1, None, None, None), lambda: tr1.invtrans_adj(1, None, None),
                 lambda: tr1.invtrans_grad_field(None, None), lambda: tr1.invtrans_adj_field(None, None)):
        with pytest.raises(NotImplementedError):
            call()


def test_unsupported_configurations_are_refused_by_name():
    lat = np.linspace(80.0, -80.0, 32)
    g = atlas_amd.StructuredGrid(nx=np.full(32, 64), y=lat)
    with pytest.raises(_lib.AtlasAmdError, match="Gaussian"):
        atlas_amd.Trans(g, 15, dirtrans=1)
    o32 = atlas_amd.Grid("O32")
    with pytest.raises(_lib.AtlasAmdError, match="rows= / domain="):
        atlas_amd.Trans(o32, 31, rows=(4, 20), dirtrans=1)
    with pytest.raises(_lib.AtlasAmdError, match="rows= / domain="):
        atlas_amd.Trans(o32, 31, domain=(0.0, 90.0, -30.0, 30.0), dirtrans=1)
    with pytest.raises(_lib.AtlasAmdError, match="nparts"):
        atlas_amd.Trans(o32, 31, nparts=2, part=0, dirtrans=1)
    with pytest.raises(_lib.AtlasAmdError, match="nparts"):
        atlas_amd.Trans(o32, 31, nparts=2, part=0, shard="mirror", dirtrans=1)
    # the four longest row lengths of O2560 do not fit a CU's LDS (a low truncation keeps the object small)
    with pytest.raises(_lib.AtlasAmdError, match="LDS"):
        atlas_amd.Trans(atlas_amd.Grid("O2560"), 63, dirtrans=1)
    # a grid given by its rows and the Gaussian latitudes of N16 is a Gaussian grid
    f16 = atlas_amd.Grid("F16")
    g = atlas_amd.StructuredGrid(nx=f16.nx(), y=f16.y())
    tr = atlas_amd.Trans(g, 31, dirtrans=1)
    sp = spectra_without_last_column(31, 1, seed=5)
    gp = np.zeros(g.size())
    tr.invtrans(1, sp, gp)
    assert np.max(np.abs(tr.dirtrans(1, gp, np.zeros_like(sp)) - sp)) <= 1e-12 * np.max(np.abs(sp))
