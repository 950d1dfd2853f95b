// Direct Legendre stage on gfx950: fp64 MFMA contraction of the inverse transform's Legendre table against the Fourier intermediate
// (legendre_dir.h).  It is the inverse stage with the wavenumber and latitude roles swapped: the latitude is the contraction index.
//
// Work decomposition: one workgroup (4 waves) per (m, 64 table rows k0 .. k0 + 63 of both parities, chunk of 16 NT columns
// r = 2 f + imag).  It walks the Legendre rows of m in 16-row chunks, always in increasing order: the summation order of a
// coefficient is fixed by (m, n) alone -- not by the field count, the column chunk or the launch -- and there are no atomics.
// Per chunk the workgroup stages G = F(north) +- F(south) for its columns in LDS (double buffered: the next chunk's loads are in
// flight during the current chunk's MFMAs); each wave keeps 16 table rows of both parities and streams them from the table,
// whose blocks [parity][kpad][64 latitudes] it reads once per column chunk.  The items of one m sit on one XCD group
// (legendre_dir.h: launch order), so the G rows a wave re-reads for its other k tiles and column chunks come from that XCD's L2.
//
// MFMA v_mfma_f64_16x16x4_f64 operand roles (as in legendre_kernel.hip):
//   A (16 x 4) = P   : lane l holds P[k = 16 w + (l & 15)][lat = 4 s + (l >> 4)]
//   B (4 x 16) = G   : lane l holds G[lat = 4 s + (l >> 4)][r = 16 j + (l & 15)]
//   D (16 x 16)      : lane l, reg g holds a[k = 16 w + (l >> 4) + 4 g][r = 16 j + (l & 15)]
#include <hip/hip_runtime.h>

#include "legendre_dir.h"

namespace atlas_amd {
namespace trans {

namespace {
typedef double d4 __attribute__((ext_vector_type(4)));
constexpr int DIR_NTHR = 256;
constexpr int LCH      = 16;   // Legendre rows per chunk
constexpr int TBN      = 64;   // latitudes per table tile (trans_plan.h: LEG_BN)
}  // namespace

template <int NT>
__global__ void __launch_bounds__(DIR_NTHR) legendre_dir_kernel(DirLegendreParams p) {
    constexpr int CW   = 16 * NT;                          // columns per workgroup
    constexpr int GSTR = CW + ((16 - CW % 32) + 32) % 32;  // LDS row stride == 16 mod 32 doubles: conflict-free ds_read_b64
    constexpr int GBUF = 2 * LCH * GSTR;                   // one buffer: sym rows, then asym rows
    constexpr int EPT  = LCH * CW / DIR_NTHR;              // staged elements per thread (= NT)
    __shared__ double G[2 * GBUF];

    const int bx    = blockIdx.x & 7;
    const int bq    = blockIdx.x >> 3;
    const int chunk = bq % p.nchunks;
    const int slot  = (bq / p.nchunks) * 8 + bx;
    if (slot >= p.nitems) {
        return;
    }
    const DirLegendreItem it = p.items[slot];
    if (it.m < 0) {
        return;
    }
    const int tid  = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int m    = it.m;
    const int c0   = chunk * CW;
    const int ncol = 2 * p.nf;
    const int nlc  = (it.L + LCH - 1) / LCH;

    d4 acc[2][NT];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[q][j] = d4{0, 0, 0, 0};

    // staging: element e of this thread is (row i, column c) = divmod(tid + 256 e, CW) of the chunk
    double gn[EPT], gs[EPT];
    auto load = [&](int lc) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int q   = tid + DIR_NTHR * e;
            const int i   = q / CW, c = q % CW;
            const int lat = lc * LCH + i;
            const int r   = c0 + c;
            const int jn  = it.nlat0 + lat;
            const int js  = p.nlats - 1 - jn;
            const bool ok = lat < it.L && r < ncol;
            gn[e]         = ok ? p.F[((long long)jn * p.m_cnt + m) * p.RP + r] : 0.;
            gs[e]         = (ok && js != jn) ? p.F[((long long)js * p.m_cnt + m) * p.RP + r] : 0.;
            if (js == jn) {   // a row on the equator counts once, and only in the symmetric sum: halves (exact) give sym = F, asym = 0
                gn[e] *= 0.5;
                gs[e] = gn[e];
            }
        }
    };
    auto store = [&](int buf) {
        double* g = G + buf * GBUF;
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int q = tid + DIR_NTHR * e;
            const int i = q / CW, c = q % CW;
            g[i * GSTR + c]         = gn[e] + gs[e];
            g[(LCH + i) * GSTR + c] = gn[e] - gs[e];
        }
    };

    // table rows of this lane (clamped: rows beyond kpad belong to no coefficient and are discarded)
    const int kl          = it.k0 + 16 * wave + (lane & 15);
    const int kc          = kl < it.kpad ? kl : it.kpad - 1;
    const long long tstep = 2ll * it.kpad * TBN;   // doubles from one latitude tile's block to the next
    const double* Pk      = p.P + it.p_off + (long long)kc * TBN;
    const bool active     = it.k0 + 16 * wave < it.kpad;   // a wave whose 16 rows are all padding only helps with the staging

    if (nlc > 0) {
        load(0);
        store(0);
    }
    __syncthreads();
    for (int lc = 0; lc < nlc; ++lc) {
        const int buf = lc & 1;
        if (lc + 1 < nlc) {
            load(lc + 1);
        }
        if (active) {
            double a[2][4];
            const int lat0 = lc * LCH + (lane >> 4);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int lat      = lat0 + 4 * s;
                const double* blk  = Pk + (long long)(lat / TBN) * tstep + (lat % TBN);
                a[0][s]            = blk[0];
                a[1][s]            = blk[(long long)it.kpad * TBN];
            }
            const double* g = G + buf * GBUF + (lane >> 4) * GSTR + (lane & 15);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const double bs = g[4 * s * GSTR + 16 * j];
                    const double ba = g[(LCH + 4 * s) * GSTR + 16 * j];
                    acc[0][j]       = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0][s], bs, acc[0][j], 0, 0, 0);
                    acc[1][j]       = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1][s], ba, acc[1][j], 0, 0, 0);
                }
            }
        }
        if (lc + 1 < nlc) {
            store(buf ^ 1);
        }
        __syncthreads();
    }
    if (!active) {
        return;
    }

    // ---- epilogue: row k of parity q is n = ntop_q - 2 k (the table's order, legendre_kernel.hip), stored in place
    const int TL    = p.T + 1;
    const int ntop0 = TL - ((TL - m) & 1);
    const int ntop1 = TL - 1 + ((TL - m) & 1);
    const long long mbase = (long long)(2 * p.T + 3 - m) * m / 2 - m;   // pos(m, n) = mbase + n
#pragma unroll
    for (int q = 0; q < 2; ++q) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int k = it.k0 + 16 * wave + (lane >> 4) + 4 * g;
            const int n = (q ? ntop1 : ntop0) - 2 * k;
            if (k >= it.kpad || n < m || n > p.T) {
                continue;
            }
            const long long pos = mbase + n;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int r = c0 + 16 * j + (lane & 15);
                if (r < ncol) {
                    const int f = r >> 1, im = r & 1;
                    p.sp[(2 * pos + im) * p.nf + f] = (m == 0 && im) ? 0. : acc[q][j][g];
                }
            }
        }
    }
}

hipError_t launch_legendre_dir(const DirLegendreParams& p, int ntile, hipStream_t stream) {
    if (p.nitems <= 0 || p.nchunks <= 0) {
        return hipSuccess;
    }
    const dim3 grid((unsigned)((p.nitems / 8) * 8 * p.nchunks));
    switch (ntile) {
        case 2: hipLaunchKernelGGL(legendre_dir_kernel<2>, grid, dim3(DIR_NTHR), 0, stream, p); break;
        case 4: hipLaunchKernelGGL(legendre_dir_kernel<4>, grid, dim3(DIR_NTHR), 0, stream, p); break;
        case 6: hipLaunchKernelGGL(legendre_dir_kernel<6>, grid, dim3(DIR_NTHR), 0, stream, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace trans
}  // namespace atlas_amd
