// C ABI of libsdfa_hip.so (include/sdfa_hip.h): audio ingest -- kaiser_best resampling (resample.hip).
#include "host.h"
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
    const int64_t n_res = (int64_t)((double)n_in * ratio);          // resampy: shape[axis] = int(shape[axis] * sample_ratio)
    if (n_res < 1) return sdfa_fail(SDFA_EINVAL, "resample: input signal length=%lld is too small to resample from %d->%d", (long long)n_in, sr_orig, sr_new);
    if (!d_workspace || workspace_bytes < n_res * 8 || ((uintptr_t)d_workspace & 7)) return sdfa_fail(SDFA_ENOSPACE, "resample: workspace too small or misaligned");
    ResampleTable tb;
    {
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
    }
    // time register: time_register += 1 / sample_ratio per output sample, accumulated sequentially in float64 like the
    // reference loop (t * increment would round differently).  Uploaded with a blocking copy: this ingest call synchronises.
    std::vector<double> treg((size_t)n_res);
    {
        const double inc = 1.0 / ratio;
        double tr = 0.0;
        for (int64_t t = 0; t < n_res; ++t) { treg[(size_t)t] = tr; tr += inc; }
    }
    HIP_TRY(hipMemcpyAsync(d_workspace, treg.data(), (size_t)n_res * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));     // the host staging vector dies with this call
    ResampleArgs a{};
    a.x = d_in; a.n_in = n_in; a.y = d_out; a.n_res = n_res; a.n_out = n_out; a.win = tb.win; a.delta = tb.delta;
    a.treg = (const double *)d_workspace; a.nwin = RS_NWIN; a.scale = ratio < 1.0 ? ratio : 1.0;
    a.step = (int64_t)(a.scale * (double)RS_TABLE); a.num_table = RS_TABLE;
    if (a.step < 1) return sdfa_fail(SDFA_EINVAL, "resample: ratio %g is too small for the filter table", ratio);
    HIP_TRY(sdfa_launch_resample(a, s));
    return SDFA_OK;
}

}  // extern "C"
