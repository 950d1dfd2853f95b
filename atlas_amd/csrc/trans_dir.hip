// Direct transform of scalar fields (an extension: TransLocal does not implement dirtrans): host orchestration of the forward
// Fourier stage (fft_fwd_kernel.hip) and the direct Legendre stage (legendre_dir_kernel.hip) on the object's stream.
//
//   F_m(j) = (1 / n_j) sum_i x_{j,i} exp(-i m lambda_i),   m <= M_j (the inverse's cut-off of row j)
//   a_n^m  = 1/2 sum_j w_j P_n^m(mu_j) F_m(j)               (w_j: Gaussian weights at the grid's own latitudes)
// The factor 1/2 is the inverse of the table's normalisation (the integral of P_n^m squared over [-1, 1] is 2); with it
// dirtrans(invtrans(s)) = s wherever the quadrature and the rows are exact.  w_j / (2 n_j) is folded into the Fourier stage's store.
#include "env.h"
#include "trans.h"
#include "fft_fwd.h"
#include "legendre_dir.h"

#include <algorithm>
#include <map>
#include <sstream>
#include <stdexcept>

namespace atlas_amd {
namespace trans {

namespace {
void dir_check(hipError_t e, const char* what) {
    if (e != hipSuccess) {
        (void)hipGetLastError();
        throw std::runtime_error(std::string("HIP error '") + hipGetErrorString(e) + "' in " + what + " (dirtrans)");
    }
}
template <typename T>
T* dir_upload(const std::vector<T>& v) {
    T* d = nullptr;
    dir_check(hipMalloc((void**)&d, std::max<size_t>(v.size(), 1) * sizeof(T)), "hipMalloc");
    if (!v.empty()) {
        dir_check(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy");
    }
    return d;
}
constexpr size_t kMaxPendingDirTimings = 1024;   // calls whose events are held before they are folded into the totals
}  // namespace

struct DirTransState {
    std::vector<double> weights;           // [nlats]
    double* d_row_scale = nullptr;         // [nlats] w_j / (2 n_j)
    fft::FftShape* d_gshape = nullptr;     // [plans]
    struct RowClass {
        int lds_bytes = 0;
        int nrows     = 0;
        int* d_rows   = nullptr;
    };
    std::vector<RowClass> classes;         // rows bucketed by LDS need (a long row's LDS does not limit the short rows' occupancy)
    DirLegendreItem* d_items = nullptr;
    int nitems               = 0;
    std::vector<hipEvent_t> events;        // profile: 3 per call (Fourier begin, Fourier end = Legendre begin, Legendre end)
    size_t ev_used = 0;
    double ms[2]   = {0, 0};
    int calls[2]   = {0, 0};

    ~DirTransState() {
        (void)hipFree(d_row_scale);
        (void)hipFree(d_gshape);
        for (RowClass& c : classes) {
            (void)hipFree(c.d_rows);
        }
        (void)hipFree(d_items);
        for (hipEvent_t e : events) {
            (void)hipEventDestroy(e);
        }
    }
    void collect(hipStream_t s) {
        if (ev_used == 0) {
            return;
        }
        dir_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        for (size_t i = 0; i + 2 < ev_used; i += 3) {
            float a = 0, b = 0;
            dir_check(hipEventElapsedTime(&a, events[i], events[i + 1]), "hipEventElapsedTime");
            dir_check(hipEventElapsedTime(&b, events[i + 1], events[i + 2]), "hipEventElapsedTime");
            ms[0] += a;
            ms[1] += b;
            calls[0]++;
            calls[1]++;
        }
        ev_used = 0;
    }
};

void Trans::enable_dirtrans(const grid::StructuredGrid& grid) {
    if (dir_) {
        return;
    }
    if (grid::gaussian_number(grid) <= 0 || grid.ny() != geo_.nlats) {
        throw std::invalid_argument("dirtrans: only global Gaussian grids (F, O or classic N) are supported; '" + grid.name +
                                    "' is not one");
    }
    if (cfg_.nparts != 1) {
        throw std::invalid_argument("dirtrans: nparts > 1 (sharded objects) is not supported; use a single-device Trans");
    }
    if (cfg_.row_end > cfg_.row_begin || windowed() || cfg_.ndgl > 0) {
        throw std::invalid_argument("dirtrans: rows= / domain= crops and mirror bands are not supported; transform the whole grid");
    }
    if (!gemm_rows_.empty()) {
        std::ostringstream ss;
        ss << "dirtrans: rows whose transform does not fit a CU's LDS are not supported (row length";
        for (const GemmRows& g : gemm_rows_) {
            ss << " " << g.n;
        }
        ss << ")";
        throw std::invalid_argument(ss.str());
    }
    for (const fft::FftRowPlan& pl : fftplans_.plans) {
        if (pl.method != fft::FFT_DIRECT && pl.method != fft::FFT_BLUESTEIN && pl.method != fft::FFT_ODD && pl.method != fft::FFT_DFT) {
            throw std::invalid_argument("dirtrans: rows planned as hybrid / native mixed-radix (experiments build switches) are not supported");
        }
    }
    auto st = std::make_shared<DirTransState>();
    const int nlats = geo_.nlats;
    st->weights.resize(nlats);
    grid::gaussian_weights(grid, st->weights.data());
    std::vector<double> scale(nlats);
    for (int j = 0; j < nlats; ++j) {
        scale[j] = 0.5 * st->weights[j] / (double)(geo_.rowoff[j + 1] - geo_.rowoff[j]);
    }
    st->d_row_scale = dir_upload(scale);

    // generic stage lists: the plans of rows with a specialised kernel carry its composite radices, which the generic passes lack
    std::vector<fft::FftShape> gshape(fftplans_.plans.size());
    for (size_t i = 0; i < gshape.size(); ++i) {
        const fft::FftRowPlan& pl = fftplans_.plans[i];
        if (pl.method != fft::FFT_DFT) {
            gshape[i] = fft::make_shape(pl.shape.M);
        }
    }
    st->d_gshape = dir_upload(gshape);

    // row classes of the Fourier stage: LDS need rounded up to a power of two (at least 4 KiB)
    std::map<int, std::pair<int, std::vector<int>>> by_lds;
    for (int j = 0; j < nlats; ++j) {
        const int jleg = j < geo_.nlatsNH ? j : nlats - 1 - j;
        if (geo_.mmax_leg[jleg] < 0) {
            continue;   // keeps no wavenumber
        }
        const int n     = geo_.regular ? geo_.nxmax : geo_.nx[j];
        const int bytes = fourier_fwd_lds_bytes(fftplans_.plans[fftplans_.plan_index(n)]);
        int key         = 4096;
        while (key < bytes) {
            key *= 2;
        }
        auto& c  = by_lds[key];
        c.first  = std::max(c.first, bytes);
        c.second.push_back(j);
    }
    for (auto& kv : by_lds) {
        DirTransState::RowClass c;
        c.lds_bytes = kv.second.first;
        c.nrows     = (int)kv.second.second.size();
        c.d_rows    = dir_upload(kv.second.second);
        st->classes.push_back(c);
    }

    // work items of the Legendre stage: (m, 64 table rows); all items of one m in one of eight lists (one XCD group each),
    // wavenumbers dealt longest-processing-time first, the lists interleaved into the launch order
    const int T = geo_.T;
    std::vector<std::vector<DirLegendreItem>> lists(8);
    std::vector<double> load(8, 0.);
    std::vector<int> ms(T + 1);
    std::vector<double> cost(T + 1);
    for (int m = 0; m <= T; ++m) {
        ms[m]   = m;
        cost[m] = double(std::max(geo_.L(m), 0) + 16) * double(num_n(T + 1, m, true));
    }
    std::sort(ms.begin(), ms.end(), [&](int a, int b) { return cost[a] > cost[b] || (cost[a] == cost[b] && a < b); });
    for (int m : ms) {
        const int x    = int(std::min_element(load.begin(), load.end()) - load.begin());
        load[x] += cost[m];
        const int kpad = (num_n(T + 1, m, true) + LEG_KB - 1) / LEG_KB * LEG_KB;
        const int L    = std::max(geo_.L(m), 0);
        long long poff = 0;
        if (L > 0) {
            const LegendreItem& first = work_.items_by_m[work_.first_item_of_m[m]];
            if (first.m != m || first.tile != 0 || first.kpad != kpad || first.p_off < 0) {
                throw std::logic_error("dirtrans: unexpected Legendre table layout");
            }
            poff = first.p_off;
        }
        for (int k0 = 0; k0 < kpad; k0 += 64) {
            lists[x].push_back(DirLegendreItem{m, k0, kpad, L, L > 0 ? geo_.nlat0[m] : 0, 0, poff});
        }
    }
    size_t maxlen = 0;
    for (auto& l : lists) {
        maxlen = std::max(maxlen, l.size());
    }
    std::vector<DirLegendreItem> items;
    for (size_t q = 0; q < maxlen; ++q) {
        for (int x = 0; x < 8; ++x) {
            items.push_back(q < lists[x].size() ? lists[x][q] : DirLegendreItem{-1, 0, 0, 0, 0, 0, 0});
        }
    }
    st->nitems  = (int)items.size();
    st->d_items = dir_upload(items);
    dir_ = st;
}

const std::vector<double>& Trans::gaussian_weights() const {
    if (!dir_) {
        throw std::logic_error("Not implemented: dirtrans (build the Trans with dirtrans=1)");
    }
    return dir_->weights;
}

void Trans::dirtrans_scalar_device(int nb_fields, const double* gp_dev, double* sp_dev) {
    if (!dir_) {
        throw std::logic_error("Not implemented: dirtrans (build the Trans with dirtrans=1)");
    }
    if (nb_fields <= 0) {
        return;
    }
    DirTransState& st = *dir_;
    const int RP      = fourier_row_pitch(nb_fields);
    double* F         = fourier_buffer(nb_fields);   // grows (with a synchronisation) only on the first call of a larger shape

    if (profile_) {
        if (st.ev_used + 3 > 3 * kMaxPendingDirTimings) {
            st.collect(stream_);
        }
        while (st.events.size() < st.ev_used + 3) {
            hipEvent_t e;
            dir_check(hipEventCreate(&e), "hipEventCreate");
            st.events.push_back(e);
        }
        dir_check(hipEventRecord(st.events[st.ev_used], stream_), "hipEventRecord");
    }
    DirFourierParams fp;
    fp.gp        = gp_dev;
    fp.npts      = geo_.npts;
    fp.nf        = nb_fields;
    fp.plans     = (const fft::FftRowPlan*)d_fftplans_;
    fp.table     = (const fft::cplx*)d_ffttable_;
    fp.gshape    = st.d_gshape;
    fp.row_plan  = d_row_plan_;
    fp.row_mmax  = d_row_mmax_;
    fp.rowoff    = d_rowoff_;
    fp.row_scale = st.d_row_scale;
    fp.F         = F;
    fp.RP        = RP;
    fp.m_cnt     = m_cnt_;
    for (const DirTransState::RowClass& c : st.classes) {
        fp.rows  = c.d_rows;
        fp.nrows = c.nrows;
        dir_check(launch_fourier_fwd(fp, c.lds_bytes, stream_), "forward Fourier stage");
    }
    if (profile_) {
        dir_check(hipEventRecord(st.events[st.ev_used + 1], stream_), "hipEventRecord");
    }
    // column tiles per workgroup: the fewest padded columns, ties to the wider tile
    int ntile = 6, best = 1 << 30;
    for (int nt : {6, 4, 2}) {
        const int cw  = 16 * nt;
        const int pad = (2 * nb_fields + cw - 1) / cw * cw;
        if (pad < best) {
            best  = pad;
            ntile = nt;
        }
    }
    DirLegendreParams lp;
    lp.P       = d_P_;
    lp.F       = F;
    lp.sp      = sp_dev;
    lp.items   = st.d_items;
    lp.nitems  = st.nitems;
    lp.nchunks = (2 * nb_fields + 16 * ntile - 1) / (16 * ntile);
    lp.T       = geo_.T;
    lp.nf      = nb_fields;
    lp.RP      = RP;
    lp.m_cnt   = m_cnt_;
    lp.nlats   = geo_.nlats;
    dir_check(launch_legendre_dir(lp, ntile, stream_), "direct Legendre stage");
    if (profile_) {
        dir_check(hipEventRecord(st.events[st.ev_used + 2], stream_), "hipEventRecord");
        st.ev_used += 3;
    }
}

void Trans::dirtrans(int nb_fields, const double gp_fields[], double scalar_spectra[]) {
    if (!dir_) {
        throw std::logic_error("Not implemented: dirtrans (build the Trans with dirtrans=1)");
    }
    if (nb_fields <= 0) {
        return;
    }
    const size_t nsp = nb_spectral_coefficients() * (size_t)nb_fields;
    const size_t ngp = (size_t)geo_.npts * (size_t)nb_fields;
    ensure(d_gp_, gp_cap_, ngp);
    ensure(d_sp_, sp_cap_, nsp);
    dir_check(hipMemcpyAsync(d_gp_, gp_fields, ngp * sizeof(double), hipMemcpyHostToDevice, stream_), "hipMemcpyAsync");
    dirtrans_scalar_device(nb_fields, d_gp_, d_sp_);
    dir_check(hipMemcpyAsync(scalar_spectra, d_sp_, nsp * sizeof(double), hipMemcpyDeviceToHost, stream_), "hipMemcpyAsync");
    synchronize();
}

void Trans::dirtrans_timings(double out[4], bool reset) {
    if (!dir_) {
        throw std::logic_error("Not implemented: dirtrans (build the Trans with dirtrans=1)");
    }
    dir_->collect(stream_);
    out[0] = dir_->ms[0];
    out[1] = dir_->calls[0];
    out[2] = dir_->ms[1];
    out[3] = dir_->calls[1];
    if (reset) {
        dir_->ms[0] = dir_->ms[1] = 0;
        dir_->calls[0] = dir_->calls[1] = 0;
    }
}

}  // namespace trans
}  // namespace atlas_amd
