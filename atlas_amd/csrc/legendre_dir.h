// Direct Legendre stage of the direct transform (legendre_dir_kernel.hip): for every zonal wavenumber m
//   a[n][r] = sum over the Legendre rows j of m (nlat0[m] <= j < nlatsLegR) of P[m][n][j] * G[m][j][r]
// with G = F(north row) + F(south row) for even n - m and F(north) - F(south) for odd n - m (the Fourier intermediate already
// carries w_j / (2 n_j)), read from the inverse transform's tile-blocked table [parity][kpad][64 latitudes] per (m, tile).
#pragma once
#include <hip/hip_runtime.h>

namespace atlas_amd {
namespace trans {

struct DirLegendreItem {   // one workgroup's rows: wavenumber m, table rows k0 .. k0 + 63 of both parities
    int m;                 // -1: padding slot of the launch order
    int k0;
    int kpad;              // table rows per parity of m (multiple of 8)
    int L;                 // Legendre rows of m (0: no latitude keeps m -- the coefficients are zero)
    int nlat0;             // first Legendre row of m
    int pad_;
    long long p_off;       // table block of the first latitude tile of m; tile t follows at p_off + t * 2 * kpad * 64
};

struct DirLegendreParams {
    const double* P;       // the inverse transform's table
    const double* F;       // Fourier intermediate F[(lat * m_cnt + m) * RP + 2 f + imag]
    double* sp;            // sp[(2 * pos(m, n) + imag) * nf + f], pos(m, n) = (2T + 3 - m) m / 2 + n - m
    const DirLegendreItem* items;   // launch order: item i runs on the XCD group i % 8
    int nitems;            // a multiple of 8
    int nchunks;           // column chunks per item
    int T, nf, RP, m_cnt, nlats;
};

// ntile: column tiles of 16 per workgroup (2, 4 or 6)
hipError_t launch_legendre_dir(const DirLegendreParams& p, int ntile, hipStream_t stream);

}  // namespace trans
}  // namespace atlas_amd
