// Forward Fourier stage of the direct transform on gfx950 (see fft_fwd.h for the method per row class).  One run-time shaped
// kernel: the row's plan is read at run time and its passes are the generic ones of fft_core.h (dif_stage_any / dit_stage_any),
// as in fft_rows_kernel.  Every (row, field) is computed by the same instruction sequence whatever the field
// count or the launch it belongs to, so a field's coefficients do not depend on nb_fields.
#include <hip/hip_runtime.h>

#include "dyn_lds.h"
#include "fft_fwd.h"

namespace atlas_amd {
namespace trans {

namespace {
constexpr int FWD_NTHR = 256;

// Y_k of the "+" direction transform of the row from the half-length transform Z held in LDS (DIRECT / BLUESTEIN rows), 0 <= k <= h
__device__ __forceinline__ fft::cplx r2c_post(const fft::cplx* work, const fft::FftRowPlan& pl, const fft::FftShape& sh,
                                              const fft::cplx* pre,
                                              const fft::cplx* chirp, int k) {
    const int h   = pl.h;
    const int k0  = k < h ? k : 0;            // Z is h-periodic
    const int k1  = k0 == 0 ? 0 : h - k0;
    fft::cplx a, b;
    if (pl.method == fft::FFT_BLUESTEIN) {    // natural order after the inverse DIT passes, times the chirp
        a = fft::cmul(work[fft::PAD(k0)], chirp[k0]);
        b = fft::cmul(work[fft::PAD(k1)], chirp[k1]);
    }
    else {                                    // digit-reversed order after the DIF passes
        a = work[fft::PAD(fft::pos_of_freq(sh, k0))];
        b = work[fft::PAD(fft::pos_of_freq(sh, k1))];
    }
    b = fft::cconj(b);
    const fft::cplx e{0.5 * (a.re + b.re), 0.5 * (a.im + b.im)};
    const fft::cplx o{0.5 * (a.im - b.im), -0.5 * (a.re - b.re)};   // (a - b) / 2i
    const fft::cplx w = k < h ? pre[k] : fft::cplx{-1., 0.};
    return fft::cadd(e, fft::cmul(w, o));
}
}  // namespace

__global__ void __launch_bounds__(FWD_NTHR) fft_fwd_rows_kernel(DirFourierParams p) {
    extern __shared__ double lds_raw[];
    fft::cplx* work = reinterpret_cast<fft::cplx*>(lds_raw);
    const int job = blockIdx.x;
    if (job >= p.nrows * p.nf) {
        return;
    }
    const int row  = p.rows[job / p.nf];
    const int f    = job % p.nf;
    const int mmax = p.row_mmax[row];
    if (mmax < 0) {
        return;   // the row keeps no wavenumber: nothing of it is ever read
    }
    const fft::FftRowPlan& pl = p.plans[p.row_plan[row]];
    const int n               = pl.n;
    const int tid             = threadIdx.x;
    const double* __restrict__ x = p.gp + (long long)f * p.npts + p.rowoff[row];
    double* __restrict__ out     = p.F + (long long)row * p.m_cnt * p.RP + 2 * f;
    const double scale           = p.row_scale[row];
    const fft::cplx* tw          = p.table + pl.off_tw;
    const fft::cplx* pre         = p.table + pl.off_pre;
    const fft::cplx* chirp       = p.table + pl.off_chirp;
    const fft::FftShape& sh      = p.gshape[p.row_plan[row]];   // generic passes (no composite radices)
    const int ns                 = sh.nstages;
    const int M                  = sh.M;

    // X_m of any m >= 0 from Y (k -> n - k by conjugate symmetry of a real row's spectrum)
    auto store = [&](int m, auto&& Y) {
        int k           = m % n;
        const bool flip = 2 * k > n;
        k               = flip ? n - k : k;
        fft::cplx X     = fft::cconj(Y(k));
        if (flip) {
            X = fft::cconj(X);
        }
        out[(long long)m * p.RP]     = X.re * scale;
        out[(long long)m * p.RP + 1] = m == 0 ? 0. : X.im * scale;
    };

    if (pl.method == fft::FFT_DFT) {
        for (int m = tid; m <= mmax; m += FWD_NTHR) {
            store(m, [&](int k) {
                fft::cplx s{0., 0.};
                for (int j = 0; j < n; ++j) {
                    const fft::cplx w = pre[(long long)j * k % n];
                    s.re += x[j] * w.re;
                    s.im += x[j] * w.im;
                }
                return s;
            });
        }
        return;
    }
    if (pl.method == fft::FFT_ODD) {
        for (int j = tid; j < n; j += FWD_NTHR) {
            work[fft::PAD(j)] = fft::cplx{x[j], 0.};
        }
        __syncthreads();
        for (int i = 0; i < ns; ++i) {
            fft::dif_stage_any(sh.radix[i], work, n, fft::stage_L(sh, i), sh.lsh[i], tw, +1, tid, FWD_NTHR);
            __syncthreads();
        }
        for (int m = tid; m <= mmax; m += FWD_NTHR) {
            store(m, [&](int k) { return work[fft::PAD(fft::pos_of_freq(sh, k))]; });
        }
        return;
    }
    // DIRECT / BLUESTEIN: pack pairs z_k = x_2k + i x_2k+1
    const int h = pl.h;
    for (int k = tid; k < h; k += FWD_NTHR) {
        const fft::cplx z{x[2 * k], x[2 * k + 1]};
        work[fft::PAD(k)] = pl.method == fft::FFT_BLUESTEIN ? fft::cmul(z, chirp[k]) : z;
    }
    if (pl.method == fft::FFT_BLUESTEIN) {
        for (int k = h + tid; k < M; k += FWD_NTHR) {
            work[fft::PAD(k)] = fft::cplx{0., 0.};
        }
        __syncthreads();
        // convolution with the chirp: forward passes, the filter spectrum, inverse passes.  The filter is stored in the DIF output
        // order of the plan's own shape (which may have the composite radices of the specialised kernels): position P of the
        // generic shape holds frequency freq_of_pos(sh, P), found in the table at pos_of_freq(pl.shape, freq)
        const fft::cplx* bhat = p.table + pl.off_bhat;
        for (int i = 0; i < ns; ++i) {
            fft::dif_stage_any(sh.radix[i], work, M, fft::stage_L(sh, i), sh.lsh[i], tw, -1, tid, FWD_NTHR);
            __syncthreads();
        }
        for (int P = tid; P < M; P += FWD_NTHR) {
            work[fft::PAD(P)] = fft::cmul(work[fft::PAD(P)], bhat[fft::pos_of_freq(pl.shape, fft::freq_of_pos(sh, P))]);
        }
        __syncthreads();
        for (int i = ns - 1; i >= 0; --i) {
            fft::dit_stage_any(sh.radix[i], work, M, fft::stage_L(sh, i), sh.lsh[i], tw, +1, tid, FWD_NTHR);
            __syncthreads();
        }
    }
    else {
        __syncthreads();
        for (int i = 0; i < ns; ++i) {
            fft::dif_stage_any(sh.radix[i], work, M, fft::stage_L(sh, i), sh.lsh[i], tw, +1, tid, FWD_NTHR);
            __syncthreads();
        }
    }
    for (int m = tid; m <= mmax; m += FWD_NTHR) {
        store(m, [&](int k) { return r2c_post(work, pl, sh, pre, chirp, k); });
    }
}

int fourier_fwd_lds_bytes(const fft::FftRowPlan& pl) {
    return pl.method == fft::FFT_DFT ? 0 : pl.lds_complex * (int)sizeof(fft::cplx);
}

hipError_t launch_fourier_fwd(const DirFourierParams& p, int lds_bytes, hipStream_t stream) {
    if (p.nrows <= 0 || p.nf <= 0) {
        return hipSuccess;
    }
    hipError_t e = ensure_dynamic_lds<fft_fwd_rows_kernel>(lds_bytes);
    if (e != hipSuccess) {
        return e;
    }
    hipLaunchKernelGGL(fft_fwd_rows_kernel, dim3((unsigned)(p.nrows * p.nf)), dim3(FWD_NTHR), (size_t)lds_bytes, stream, p);
    return hipGetLastError();
}

}  // namespace trans
}  // namespace atlas_amd
