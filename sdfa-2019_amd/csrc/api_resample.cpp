// C ABI of libsdfa_hip.so: audio ingest -- kaiser_best resampling (resample.hip), of a whole clip (include/sdfa_hip.h sdfa_resample)
// and of live streams at a capture rate (include/sdfa_stream.h sdfa_stream_resample*).
#include "host.h"
#include "../../include/sdfa_stream.h"
#include "kernels.h"

#include <array>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

namespace {

double bessel_i0(double x) {   // modified Bessel function of the first kind, order 0: sum_k ((x/2)^k / k!)^2
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}

constexpr int RS_ZEROS = 64, RS_TABLE = 512;                       // resampy kaiser_best: num_zeros, 2**precision
constexpr double RS_BETA = 14.769656459379492, RS_ROLLOFF = 0.9475937167399596;
constexpr int64_t RS_NWIN = (int64_t)RS_ZEROS * RS_TABLE + 1;

// right half of the Kaiser-windowed sinc (resampy/filters.py sinc_window with scipy.signal.kaiser)
void kaiser_best_half(std::vector<double> &win) {
    const int64_t n = RS_NWIN - 1;
    win.resize(RS_NWIN);
    const double i0b = bessel_i0(RS_BETA);
    for (int64_t j = 0; j <= n; ++j) {
        const double xz = RS_ROLLOFF * ((double)j / (double)RS_TABLE);                 // rolloff * linspace(0, 64, n + 1)[j]
        const double py = M_PI * (xz == 0.0 ? 1.0e-20 : xz);                           // np.sinc
        const double sinc = RS_ROLLOFF * (std::sin(py) / py);
        const double r = (double)j / (double)n;                                        // (k - alpha) / alpha, k = n + j
        const double taper = bessel_i0(RS_BETA * std::sqrt(1.0 - r * r)) / i0b;
        win[j] = taper * sinc;
    }
}

struct ResampleTable { void *blob = nullptr; const double *win, *delta; };
std::mutex g_rs_mu;
std::map<std::array<int, 3>, ResampleTable> g_rs;

// How a rate pair walks the filter: resampy's sample_ratio, min(1, ratio) and the table entries per input sample.
struct RatePlan { double ratio, scale; int64_t step; };
int rate_plan(int sr_orig, int sr_new, RatePlan &p) {
    p.ratio = (double)sr_new / (double)sr_orig;
    p.scale = p.ratio < 1.0 ? p.ratio : 1.0;
    p.step = (int64_t)(p.scale * (double)RS_TABLE);
    if (p.step < 1) return sdfa_fail(SDFA_EINVAL, "resample: ratio %g is too small for the filter table", p.ratio);
    return SDFA_OK;
}

// The filter of a rate pair on the current device (scaled by the ratio when downsampling, then its forward differences), built and
// uploaded with a blocking copy by the first call that asks for it.
int resample_table(int sr_orig, int sr_new, double ratio, ResampleTable &tb) {
    std::lock_guard<std::mutex> lk(g_rs_mu);
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const std::array<int, 3> key{sr_orig, sr_new, dev};
    auto it = g_rs.find(key);
    if (it == g_rs.end()) {
        std::vector<double> win, both(2 * RS_NWIN, 0.0);
        kaiser_best_half(win);
        for (int64_t j = 0; j < RS_NWIN; ++j) both[j] = ratio < 1.0 ? win[j] * ratio : win[j];     // interp_win *= sample_ratio
        for (int64_t j = 0; j + 1 < RS_NWIN; ++j) both[RS_NWIN + j] = both[j + 1] - both[j];       // interp_delta[:-1] = np.diff(interp_win)
        ResampleTable t;
        HIP_TRY(hipMalloc(&t.blob, both.size() * 8));
        HIP_TRY(hipMemcpy(t.blob, both.data(), both.size() * 8, hipMemcpyHostToDevice));
        t.win = (const double *)t.blob; t.delta = t.win + RS_NWIN;
        it = g_rs.emplace(key, t).first;
    }
    tb = it->second;
    return SDFA_OK;
}

// Time register of `count` consecutive outputs from the carried value `tr` (the register of the first of them; 0 for output 0):
// time_register += 1 / sample_ratio per output sample, accumulated sequentially in float64 like the reference loop (t * increment
// would round differently).  The one place both the offline call and the live streams take their registers from.
void time_register(double &tr, double inc, int64_t count, double *out) {
#pragma clang fp contract(off)
    for (int64_t i = 0; i < count; ++i) { if (out) out[i] = tr; tr += inc; }
}

// Lengths of the offline conversion of n_in samples: n_res filtered outputs (resampy: int(n * ratio)), then zeros up to the returned
// n_out = ceil(n * ratio) (librosa fix_length); the offline call's refusals.
int64_t resample_lengths(int64_t n_in, int sr_orig, int sr_new, int64_t &n_res) {
    const int64_t n_out = sdfa_resample_out_len(n_in, sr_orig, sr_new);
    if (n_out < 0) return n_out;
    n_res = n_in;
    if (sr_orig == sr_new) return n_out;
    n_res = (int64_t)((double)n_in * ((double)sr_new / (double)sr_orig));      // resampy: shape[axis] = int(shape[axis] * sample_ratio)
    if (n_res < 1) return sdfa_fail(SDFA_EINVAL, "resample: input signal length=%lld is too small to resample from %d->%d", (long long)n_in, sr_orig, sr_new);
    return n_out;
}

// Input samples that must have arrived before output `tr` is final: n + 1 + the taps of its right wing (resample_taps in resample.hip,
// wing 1, with the same float64 operations).
int64_t samples_needed(double tr, const RatePlan &p) {
#pragma clang fp contract(off)
    const int64_t n = (int64_t)tr;
    const double frac = p.scale * (tr - (double)n);
    const double right = p.scale - frac;
    const double index_frac = right * (double)RS_TABLE;
    const int64_t offset = (int64_t)index_frac;
    return n + 1 + (RS_NWIN - offset) / p.step;
}

// Registers of outputs 0, 1024, 2048, ... per rate pair, extended on demand: the register is a sequential sum, so a stateless
// question about output t (sdfa_stream_resample_final) starts from the checkpoint below it.
constexpr int64_t RS_CHECK = 1024;
std::mutex g_reg_mu;
std::map<std::array<int, 2>, std::vector<double>> g_reg;
double register_of(int64_t t, int sr_orig, int sr_new, double inc) {
    double tr;
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        std::vector<double> &cp = g_reg[{sr_orig, sr_new}];
        if (cp.empty()) cp.push_back(0.0);
        while ((int64_t)cp.size() <= t / RS_CHECK) {
            double next = cp.back();
            time_register(next, inc, RS_CHECK, nullptr);
            cp.push_back(next);
        }
        tr = cp[(size_t)(t / RS_CHECK)];
    }
    time_register(tr, inc, t % RS_CHECK, nullptr);
    return tr;
}

}  // namespace

extern "C" {

int64_t sdfa_resample_out_len(int64_t n_in, int sr_orig, int sr_new) {
    if (n_in <= 0 || sr_orig <= 0 || sr_new <= 0) return sdfa_fail(SDFA_EINVAL, "resample_out_len: bad argument");
    if (sr_orig == sr_new) return n_in;
    const double ratio = (double)sr_new / (double)sr_orig;
    return (int64_t)std::ceil((double)n_in * ratio);                // librosa.resample: n_samples = int(np.ceil(y.shape[-1] * ratio))
}

int64_t sdfa_resample_workspace_bytes(int64_t n_in, int sr_orig, int sr_new) {
    const int64_t n = sdfa_resample_out_len(n_in, sr_orig, sr_new);
    return n < 0 ? n : round_up(n * 8, 256);
}

int sdfa_resample_filter(double *h_half_window, int64_t cap) {
    if (!h_half_window || cap < RS_NWIN) return sdfa_fail(SDFA_EINVAL, "resample_filter: need room for %lld doubles", (long long)RS_NWIN);
    std::vector<double> w;
    kaiser_best_half(w);
    memcpy(h_half_window, w.data(), RS_NWIN * 8);
    return (int)RS_NWIN;
}

int sdfa_resample(const float *d_in, int64_t n_in, int sr_orig, int sr_new, float *d_out, int64_t n_out, void *d_workspace,
                  int64_t workspace_bytes, void *stream) {
    if (!d_in || !d_out || n_in <= 0 || sr_orig <= 0 || sr_new <= 0) return sdfa_fail(SDFA_EINVAL, "resample: bad argument");
    if (n_out != sdfa_resample_out_len(n_in, sr_orig, sr_new))
        return sdfa_fail(SDFA_EINVAL, "resample: n_out must be sdfa_resample_out_len() = %lld", (long long)sdfa_resample_out_len(n_in, sr_orig, sr_new));
    hipStream_t s = (hipStream_t)stream;
    if (sr_orig == sr_new) { HIP_TRY(hipMemcpyAsync(d_out, d_in, (size_t)n_in * 4, hipMemcpyDeviceToDevice, s)); return SDFA_OK; }
    const double ratio = (double)sr_new / (double)sr_orig;
    int64_t n_res = 0;
    if (int64_t rc = resample_lengths(n_in, sr_orig, sr_new, n_res); rc < 0) return (int)rc;
    if (!d_workspace || workspace_bytes < n_res * 8 || ((uintptr_t)d_workspace & 7)) return sdfa_fail(SDFA_ENOSPACE, "resample: workspace too small or misaligned");
    ResampleTable tb;
    if (int rc = resample_table(sr_orig, sr_new, ratio, tb)) return rc;
    // Uploaded with a blocking copy: this ingest call synchronises.
    std::vector<double> treg((size_t)n_res);
    double tr = 0.0;
    time_register(tr, 1.0 / ratio, n_res, treg.data());
    HIP_TRY(hipMemcpyAsync(d_workspace, treg.data(), (size_t)n_res * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));     // the host staging vector dies with this call
    ResampleArgs a{};
    a.x = d_in; a.n_in = n_in; a.y = d_out; a.n_res = n_res; a.n_out = n_out; a.win = tb.win; a.delta = tb.delta;
    RatePlan plan;
    if (int rc = rate_plan(sr_orig, sr_new, plan)) return rc;
    a.treg = (const double *)d_workspace; a.nwin = RS_NWIN; a.scale = plan.scale; a.step = plan.step; a.num_table = RS_TABLE;
    HIP_TRY(sdfa_launch_resample(a, s));
    return SDFA_OK;
}

// ------------------------------------------------------------------------------------------------
// Live streams at a capture rate (include/sdfa_stream.h)
int64_t sdfa_stream_resample_final(int64_t n_in, int sr_in, int sr_out) {
    if (n_in < 0 || n_in > ((int64_t)1 << 34) || sr_in <= 0 || sr_out <= 0) return sdfa_fail(SDFA_EINVAL, "stream_resample_final: bad argument");
    if (sr_in == sr_out) return n_in;
    RatePlan p;
    if (int rc = rate_plan(sr_in, sr_out, p)) return rc;
    const double inc = 1.0 / p.ratio;
    const int64_t widest = RS_NWIN / p.step;                        // the longest right wing
    // start below the answer: every output up to t is final when n(t) + 1 + widest <= n_in, n(t) not decreasing in t
    int64_t t = (int64_t)((double)(n_in > widest + 2 ? n_in - widest - 2 : 0) * p.ratio) - 64;
    if (t < 0) t = 0;
    double tr = register_of(t, sr_in, sr_out, inc);
    while (t > 0 && (int64_t)tr + 1 + widest > n_in) {
        t = t > RS_CHECK ? t - RS_CHECK : 0;
        tr = register_of(t, sr_in, sr_out, inc);
    }
    while (samples_needed(tr, p) <= n_in) time_register(tr, inc, 1, nullptr), ++t;      // the first output that is not final
    return t;
}

int64_t sdfa_stream_resample_register(int64_t count, int sr_in, int sr_out, double *h_state, double *h_treg) {
    if (count < 0 || sr_in <= 0 || sr_out <= 0 || !h_state) return sdfa_fail(SDFA_EINVAL, "stream_resample_register: bad argument");
    time_register(*h_state, 1.0 / ((double)sr_out / (double)sr_in), count, h_treg);
    return count;
}

int64_t sdfa_stream_resample_close(int64_t n_in, int sr_in, int sr_out, int64_t *h_n_res) {
    int64_t n_res = 0;
    const int64_t n_out = resample_lengths(n_in, sr_in, sr_out, n_res);
    if (n_out < 0) return n_out;
    if (sr_in != sr_out) { RatePlan p; if (int rc = rate_plan(sr_in, sr_out, p)) return rc; }
    if (h_n_res) *h_n_res = n_res;
    return n_out;
}

int64_t sdfa_stream_resample_wing(int sr_in, int sr_out) {
    if (sr_in <= 0 || sr_out <= 0) return sdfa_fail(SDFA_EINVAL, "stream_resample_wing: bad argument");
    if (sr_in == sr_out) return 0;
    RatePlan p;
    if (int rc = rate_plan(sr_in, sr_out, p)) return rc;
    return RS_NWIN / p.step;
}

int sdfa_stream_resample(const float *d_in_rings, int r_in, int32_t n_in_rings, float *d_rings, int r, int32_t n_rings, const int64_t *d_seg,
                         int32_t n_seg, int64_t max_count, const double *d_treg, int64_t n_treg, const int32_t *h_rates, int32_t n_rates,
                         int sr_out, void *stream) {
    if (n_seg == 0 || max_count == 0) return SDFA_OK;
    if (!d_in_rings || !d_rings || !d_seg || !h_rates || n_seg < 0 || n_seg > 65535 || max_count < 0 || n_in_rings <= 0 || n_rings <= 0 || n_treg < 0 ||
        (n_treg > 0 && !d_treg) || r < 1 || r > 28 || r_in < 1 || r_in > 28 || max_count > ((int64_t)1 << r) || sr_out <= 0)
        return sdfa_fail(SDFA_EINVAL, "stream_resample: null pointer or bad count");
    if (n_rates < 1 || n_rates > SDFA_STREAM_MAX_RATES) return sdfa_fail(SDFA_EINVAL, "stream_resample: 1 .. %d input rates per call", SDFA_STREAM_MAX_RATES);
    static_assert(SDFA_STREAM_MAX_RATES == STREAM_MAX_RATES && SDFA_STREAM_RING_MIRROR == STREAM_RING_MIRROR, "sdfa_stream.h and kernels.h disagree");
    StreamResampleArgs a{};
    for (int i = 0; i < n_rates; ++i) {
        if (h_rates[i] <= 0) return sdfa_fail(SDFA_EINVAL, "stream_resample: bad input rate %d", h_rates[i]);
        if (h_rates[i] == sr_out) continue;                          // step 0: a copy, as the offline call
        RatePlan p;
        if (int rc = rate_plan(h_rates[i], sr_out, p)) return rc;
        ResampleTable tb;
        if (int rc = resample_table(h_rates[i], sr_out, p.ratio, tb)) return rc;
        a.rate[i].win = tb.win; a.rate[i].step = p.step; a.rate[i].scale = p.scale;
    }
    a.in_rings = d_in_rings; a.rings = d_rings; a.r_in = r_in; a.n_in_rings = n_in_rings; a.r = r; a.n_rings = n_rings;
    a.seg = d_seg; a.treg = d_treg; a.n_treg = n_treg; a.nwin = RS_NWIN; a.num_table = RS_TABLE; a.n_rates = n_rates;
    HIP_TRY(sdfa_launch_stream_resample(a, n_seg, max_count, (hipStream_t)stream));
    return SDFA_OK;
}

}  // extern "C"
