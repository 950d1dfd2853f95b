// Forward (real-to-complex) Fourier stage of the direct transform: one workgroup per (latitude row, field) reads the row's grid
// points, transforms them in LDS with the passes of fft_core.h and the tables of the inverse transform's plans (fft_plan.h), and
// stores the kept wavenumbers m <= M_j, scaled, into the Fourier intermediate F[(lat * m_cnt + m) * RP + 2 f + imag].
//
// The grid points are real, so X_m = sum_i x_i exp(-2 pi i m i / n) = conj(Y_m) with Y_m the "+" direction transform the
// inverse's tables are built for:
//   DIRECT    z_k = x_2k + i x_2k+1 (h points), DIF passes in the + direction (natural order in, digit-reversed out), then the
//             r2c post-processing  Y_k = E_k + w_n^k O_k  with E_k = (Z_k + conj Z_h-k) / 2, O_k = (Z_k - conj Z_h-k) / 2i and
//             the c2r table w_n^k = exp(+2 pi i k / n)
//   BLUESTEIN the same, with the half-length transform done as the inverse's chirp-z convolution (chirp, DIF, filter, DIT,
//             chirp): the DFT matrix is symmetric, so the inverse's pipeline computes the + direction transform of any input
//   ODD       complex transform of length n of (x_i, 0), DIF passes in the + direction
//   DFT       direct sum with the table exp(+2 pi i j / n)
// Rows planned as HYBRID / NATIVE (experiments build only) are refused when the direct transform is enabled.
#pragma once
#include <hip/hip_runtime.h>

#include "fft_core.h"
#include "fft_plan.h"

namespace atlas_amd {
namespace trans {

struct DirFourierParams {
    const double* gp;                 // gp[f * npts + rowoff[row] + i]
    long long npts;
    int nf;
    const fft::FftRowPlan* plans;     // the inverse transform's device plans and tables
    const fft::cplx* table;
    const fft::FftShape* gshape;      // [plans] generic stage list of each plan's transform length (make_shape(M))
    const int* row_plan;              // [nlats]
    const int* row_mmax;              // [nlats] highest kept wavenumber (-1: none), the inverse's cut-off
    const long long* rowoff;          // [nlats + 1]
    const double* row_scale;          // [nlats] w_j / (2 n_j): quadrature weight, 1 / n_j and the 1/2 of the normalisation
    const int* rows;                  // rows of this launch
    int nrows;
    double* F;                        // Fourier intermediate
    int RP;
    int m_cnt;
};

// one launch for the rows `p.rows`; lds_bytes: the largest LDS need of those rows
hipError_t launch_fourier_fwd(const DirFourierParams& p, int lds_bytes, hipStream_t stream);
// LDS bytes the forward kernel needs for a row with this plan (0: no LDS)
int fourier_fwd_lds_bytes(const fft::FftRowPlan& pl);

}  // namespace trans
}  // namespace atlas_amd
