// C ABI of libsdfa_hip.so (include/sdfa_hip.h, include/sdfa_stream.h): the mel front end -- constants cache, frame enumeration,
// the offline calls and the live-stream rings.
#include "../../include/sdfa_stream.h"
#include "host.h"
#include "kernels.h"

#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

// A/B options this file reads (api_core.cpp)
extern thread_local int g_sdfa_mel_fft_radix4, g_sdfa_frontend_two_kernel, g_sdfa_frontend_t_major;
extern thread_local int g_sdfa_frontend_stream_block, g_sdfa_frontend_stream_slots, g_sdfa_frontend_stream_spin_max, g_sdfa_frontend_stream_phases;

namespace {

// ------------------------------------------------------------------------------------------------
// front-end constants (window, twiddles, sparse mel rows), cached per sample rate
// ------------------------------------------------------------------------------------------------
struct FrontendCache {
    FrontendConsts c{};
    void *blob = nullptr;
};
std::mutex g_fe_mu;
std::map<int, FrontendCache> g_fe;

// Slaney mel scale / triangular filters as librosa 0.8.0 filters.mel(norm="slaney") defines them
// (third-party, un-vendored; called at saber/data/audio/features/misc.py:110-117).
double hz_to_mel(double f) {
    const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
double mel_to_hz(double m) {
    const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}

int build_frontend(int sr, FrontendCache &fc) {
    const int win = (int)(0.064 * sr), hop = (int)(0.008 * sr);
    if (!((sr == 8000 && win == 512) || (sr == 16000 && win == 1024)))
        return sdfa_fail(SDFA_EINVAL, "sample_rate %d unsupported: the FFT kernels cover 8000 (win 512) and 16000 (win 1024)", sr);
    const int nbins = win / 2 + 1, n_mels = 128;
    const double fmin = 50.0, fmax = 3600.0;
    std::vector<float> hamm(win);
    std::vector<float> tw(2 * win);
    for (int n = 0; n < win; ++n) {
        hamm[n] = (float)(0.54 - 0.46 * std::cos(2.0 * M_PI * n / (win - 1)));   // np.hamming, misc.py:94-100
        tw[2 * n] = (float)std::cos(-2.0 * M_PI * n / win);
        tw[2 * n + 1] = (float)std::sin(-2.0 * M_PI * n / win);
    }
    std::vector<double> mel_f(n_mels + 2);
    const double m_lo = hz_to_mel(fmin), m_hi = hz_to_mel(fmax);
    for (int i = 0; i < n_mels + 2; ++i) mel_f[i] = mel_to_hz(m_lo + (m_hi - m_lo) * i / (n_mels + 1));
    // sparse mel rows in a fixed-width form: a band's non-zero bins are consecutive (triangular filters), the widest
    // band has 8 of them -- first bin + 8 weights (zero padded), so the kernels' band loop unrolls
    std::vector<int> bin0(n_mels, 0);
    std::vector<float> w8((size_t)8 * n_mels, 0.f);
    int used = 0, nnz = 0;
    for (int i = 0; i < n_mels; ++i) {
        const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
        int first = -1, last = -1;
        std::vector<float> row(nbins, 0.f);
        for (int b = 0; b < nbins; ++b) {
            const double fr = (double)sr / 2 * b / (nbins - 1);
            const double lower = -(mel_f[i] - fr) / (mel_f[i + 1] - mel_f[i]);
            const double upper = (mel_f[i + 2] - fr) / (mel_f[i + 2] - mel_f[i + 1]);
            const float w = (float)std::fmax(0.0, std::fmin(lower, upper));
            const float wn = (float)((double)w * enorm);   // float32 weights *= float64 enorm -> float32
            row[b] = wn;
            if (wn != 0.f) { if (first < 0) first = b; last = b; ++nnz; }
        }
        if (first < 0) { first = 0; last = 0; }             // an empty band (none at these settings): all-zero taps
        if (last - first + 1 > 8) return sdfa_fail(SDFA_EINVAL, "mel band %d spans %d bins: the kernels hold 8 taps per band", i, last - first + 1);
        for (int b = first; b <= last; ++b)
            if (row[b] == 0.f) return sdfa_fail(SDFA_EINVAL, "mel band %d is not contiguous", i);
        bin0[i] = first;
        for (int e = 0; e < 8 && first + e < nbins; ++e) w8[(size_t)e * n_mels + i] = (first + e <= last) ? row[first + e] : 0.f;
        if (last + 1 > used) used = last + 1;
    }
    // the kernels keep 256 power bins per column and read 8 taps from a band's first bin on
    for (int i = 0; i < n_mels; ++i)
        if (bin0[i] + 8 > 256) return sdfa_fail(SDFA_EINVAL, "mel filterbank does not fit the kernel tables (band %d starts at bin %d)", i, bin0[i]);
    const size_t o_h = 0, o_t = o_h + win * 4, o_p = o_t + win * 8, o_w = o_p + 128 * 4, total = o_w + 1024 * 4;
    std::vector<char> host(total, 0);
    memcpy(&host[o_h], hamm.data(), win * 4);
    memcpy(&host[o_t], tw.data(), win * 8);
    memcpy(&host[o_p], bin0.data(), bin0.size() * 4);
    memcpy(&host[o_w], w8.data(), w8.size() * 4);
    HIP_TRY(hipMalloc(&fc.blob, total));
    HIP_TRY(hipMemcpy(fc.blob, host.data(), total, hipMemcpyHostToDevice));
    char *d = (char *)fc.blob;
    fc.c.hamm = (const float *)(d + o_h);
    fc.c.twiddle = (const float2 *)(d + o_t);
    fc.c.mel_bin0 = (const int *)(d + o_p);
    fc.c.mel_w8 = (const float *)(d + o_w);
    fc.c.win = win; fc.c.hop = hop; fc.c.sliding = hop * 63 + win;
    fc.c.nbins_used = used; fc.c.nnz = nnz;
    return SDFA_OK;
}

// The constants of `sample_rate` on the current device: built on first use, then cached.
int frontend_consts(int sample_rate, FrontendConsts &c) {
    std::lock_guard<std::mutex> lk(g_fe_mu);
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    auto key = sample_rate * 64 + dev;
    auto it = g_fe.find(key);
    if (it == g_fe.end()) {
        FrontendCache fc;
        int rc = build_frontend(sample_rate, fc);
        if (rc) return rc;
        it = g_fe.emplace(key, fc).first;
    }
    c = it->second.c;
    return SDFA_OK;
}

// Frame idx + 1 of sdfa_frame_index, a function of idx alone (the loop there counts idx up from -1.0 in exact steps of 1.0).
struct FramePos { float fs; int64_t s, e; int32_t ts; };
FramePos frame_pos(double idx, int sample_rate, int fps, int64_t sliding, int ts_delta_ms) {
    FramePos f;
    // frame_to_sample: np.float32(float(idx * sr) / float(fps))          speech_anime.py:141-145
    f.fs = (float)((idx * (double)sample_rate) / (double)fps);
    const int64_t mid = (int64_t)std::floor((double)f.fs);
    f.e = mid + sliding / 2; f.s = f.e - sliding;
    // sample_to_ms: np.float32(float(((s+e)/2) * 1000.0) / float(sr)); then float32 - ts_delta; round half even
    const float ms = (float)(((((double)(f.s + f.e)) / 2.0) * 1000.0) / (double)sample_rate);
    const float shifted = ms - (float)ts_delta_ms;
    f.ts = (int32_t)std::nearbyintf(shifted);
    return f;
}

}  // namespace

int sdfa_frontend_consts(int sample_rate, FrontendConsts &c) { return frontend_consts(sample_rate, c); }

extern "C" {

// ------------------------------------------------------------------------------------------------
int64_t sdfa_frame_index(int64_t n_samples, int sample_rate, int fps, int win, int hop, int ts_delta_ms,
                         int64_t *h_starts, int32_t *h_tslist, int64_t cap) {
    if (n_samples <= 0 || sample_rate <= 0 || fps <= 0 || win <= 0 || hop <= 0) return sdfa_fail(SDFA_EINVAL, "bad frame_index arguments");
    // the front-end kernels index a clip's samples in 32-bit arithmetic (|index| < 2^29: frontend.hip); refuse longer clips here,
    // where the length is known on the host (9 h at 16 kHz; the reference's float32 frame arithmetic is exact only up to 2^24)
    if (n_samples > 0x1fffffff) return sdfa_fail(SDFA_EINVAL, "frame_index: clips of more than 2^29 - 1 samples are not supported (%lld given)", (long long)n_samples);
    const int64_t sliding = (int64_t)hop * 63 + win;
    int64_t count = 0;
    double idx = -1.0;
    for (;;) {
        const FramePos f = frame_pos(idx, sample_rate, fps, sliding, ts_delta_ms);
        // frame_in_range: float32 + int -> float32                           sliding_window.py:320-322
        const float lhs = f.fs + (float)sliding;
        if (!((double)lhs <= (double)(n_samples + 2 * sliding))) break;
        const int64_t s = f.s, e = f.e;
        const int32_t ts = f.ts;
        const int64_t lo = s > 0 ? s : 0, hi = e < n_samples ? e : n_samples;
        if (hi > lo && s < 0 && e > n_samples)
            return sdfa_fail(SDFA_ESHORTCLIP, "signal length %lld != %lld.", (long long)(hi - lo - s), (long long)sliding);
        if (count < cap) {
            if (h_starts) h_starts[count] = s;
            if (h_tslist) h_tslist[count] = ts;
        }
        ++count;
        idx += 1.0;
    }
    if (cap > 0 && count > cap) return sdfa_fail(SDFA_ENOSPACE, "frame_index: %lld frames, capacity %lld", (long long)count, (long long)cap);
    return count;
}

// ------------------------------------------------------------------------------------------------
int sdfa_mel_frontend(const float *d_pcm, const int64_t *d_clip_off, const int64_t *d_clip_len, int32_t n_clips,
                      const int32_t *d_frame_clip, const int64_t *d_frame_start, int64_t n_frames, int sample_rate,
                      float *d_audio_feat, void *stream) {
    if (n_frames == 0) return SDFA_OK;
    if (!d_pcm || !d_clip_off || !d_clip_len || !d_frame_clip || !d_frame_start || !d_audio_feat || n_clips <= 0 || n_frames < 0)
        return sdfa_fail(SDFA_EINVAL, "mel_frontend: null pointer or bad count");
    FrontendConsts c;
    if (int rc = frontend_consts(sample_rate, c)) return rc;
    HIP_TRY(sdfa_launch_frontend(c, d_pcm, d_clip_off, d_clip_len, d_frame_clip, d_frame_start, n_frames, d_audio_feat,
                                 (hipStream_t)stream));
    return SDFA_OK;
}

// ------------------------------------------------------------------------------------------------
// "spectral gather" form of the front end (frontend.hip): share map over mel columns -> FFT + mel of the distinct
// columns -> per-frame gather.  Scratch: the map (ints) followed by the mel table (128 floats per column, sized for the
// case that nothing is shared).
namespace {
struct FeWs { int64_t Nc, Mc, map_ints, table_off, total; };
FeWs fe_layout(int64_t n_frames) {
    FeWs w;
    w.Nc = round_up(n_frames, 128); w.Mc = 64 * w.Nc;
    w.map_ints = round_up(sdfa_share_table_words(w.Nc) + 1, 64);
    w.table_off = w.map_ints * 4;
    w.total = w.table_off + w.Mc * 128 * 4;
    return w;
}
}  // namespace

// The spectral-stream kernel's status word of the LAST sdfa_mel_frontend_gather call on this workspace: bounded hand-off waits that
// expired (0 always, unless the producer / consumer form's logic is wrong) -- the repair pass behind the kernel redid such a call, the features are right
// either way.  Synchronises the stream.  Tests only.
int sdfa_debug_frontend_status(const void *d_workspace, void *stream) {
    if (!d_workspace) return sdfa_fail(SDFA_EINVAL, "frontend_status: null workspace");
    int32_t v = 0;
    HIP_TRY(hipMemcpyAsync(&v, reinterpret_cast<const int32_t *>(d_workspace) + 8, sizeof v, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return (int)v;
}

int64_t sdfa_frontend_workspace_bytes(int64_t max_frames) {
    if (max_frames <= 0) return sdfa_fail(SDFA_EINVAL, "frontend_workspace_bytes: bad argument");
    return fe_layout(max_frames).total;
}

int sdfa_mel_frontend_gather(const float *d_pcm, const int64_t *d_clip_off, const int64_t *d_clip_len, int32_t n_clips,
                             const int32_t *d_frame_clip, const int64_t *d_frame_start, int64_t n_frames, int sample_rate,
                             float *d_audio_feat, void *d_workspace, int64_t workspace_bytes, void *stream) {
    if (n_frames == 0) return SDFA_OK;
    if (!d_pcm || !d_clip_off || !d_clip_len || !d_frame_clip || !d_frame_start || !d_audio_feat || !d_workspace || n_clips <= 0 || n_frames < 0)
        return sdfa_fail(SDFA_EINVAL, "mel_frontend_gather: null pointer or bad count");
    if (((uintptr_t)d_workspace | (uintptr_t)d_audio_feat) & 15) return sdfa_fail(SDFA_EINVAL, "mel_frontend_gather: pointers must be 16-byte aligned");
    const FeWs w = fe_layout(n_frames);
    if (workspace_bytes < w.total)
        return sdfa_fail(SDFA_ENOSPACE, "mel_frontend_gather: workspace of %lld bytes, %lld needed for %lld frames", (long long)workspace_bytes,
                    (long long)w.total, (long long)n_frames);
    if (w.Mc >= (int64_t)1 << 31) return sdfa_fail(SDFA_EINVAL, "mel_frontend_gather: too many frames in one call");
    FrontendConsts c;
    if (int rc = frontend_consts(sample_rate, c)) return rc;
    hipStream_t s = (hipStream_t)stream;
    int32_t *sh = reinterpret_cast<int32_t *>(d_workspace);
    ShareArgs sa{};
    sa.frame_clip = d_frame_clip; sa.frame_start = d_frame_start; sa.hop = c.hop;
    sa.t_lo = 1; sa.t_hi = 63;          // every window column but the first (raw first sample) is a function of (clip, position)
    sa.frame_major = g_sdfa_frontend_t_major ? 0 : 1;      // distinct columns numbered clip by clip, hop by hop, per-column arrays indexed [n][t] (share.hip: col_index)
    sa.N = n_frames; sa.Nc = w.Nc; sa.Mc = w.Mc;
    sdfa_share_carve(sa, sh);
    // sh[8]: the stream kernel's status word (bounded hand-off waits that expired -- never, unless its logic is wrong -- and were
    // repaired by the pass behind the kernel).  Zeroed by EVERY call, whichever form runs, so that sdfa_debug_frontend_status never
    // reads a stale or uninitialised word after a two-kernel / radix-4 / t-major call or on a fresh workspace.
    HIP_TRY(hipMemsetAsync(sh + 8, 0, sizeof(int32_t), s));
    if (!g_sdfa_frontend_two_kernel && !g_sdfa_mel_fft_radix4 && !g_sdfa_frontend_t_major) {
        // spectral stream (frontend.hip): the chains are read from prev / shift, the mel rows live in an LDS ring, no table
        HIP_TRY(sdfa_launch_share_prev(sa, s));
        HIP_TRY(sdfa_launch_mel_stream(c, d_pcm, d_clip_off, d_clip_len, d_frame_clip, d_frame_start, sa.prev, sa.shift, n_frames,
                                       g_sdfa_frontend_stream_block, g_sdfa_frontend_stream_slots, g_sdfa_frontend_stream_phases ? 0 : 1, g_sdfa_frontend_stream_spin_max, sh + 8, d_audio_feat, s));
        return SDFA_OK;
    }
    HIP_TRY(sdfa_launch_share_map(sa, s));
    float *table = reinterpret_cast<float *>(reinterpret_cast<char *>(d_workspace) + w.table_off);
    HIP_TRY(sdfa_launch_mel_columns(c, d_pcm, d_clip_off, d_clip_len, d_frame_clip, d_frame_start, sa.col_src, sa.counts, table, s));
    HIP_TRY(sdfa_launch_gather_features(table, sa.col_to_u, n_frames, w.Nc, sa.frame_major, d_audio_feat, s));
    return SDFA_OK;
}

// ------------------------------------------------------------------------------------------------
// Live streams (include/sdfa_stream.h)
int64_t sdfa_stream_frame_positions(int64_t k0, int64_t count, int sample_rate, int fps, int win, int hop, int ts_delta_ms,
                                    int64_t *h_starts, int32_t *h_tslist) {
    if (k0 < 0 || count < 0 || sample_rate <= 0 || fps <= 0 || win <= 0 || hop <= 0) return sdfa_fail(SDFA_EINVAL, "bad stream_frame_positions arguments");
    const int64_t sliding = (int64_t)hop * 63 + win;
    for (int64_t i = 0; i < count; ++i) {
        const FramePos f = frame_pos((double)(k0 + i) - 1.0, sample_rate, fps, sliding, ts_delta_ms);
        if (h_starts) h_starts[i] = f.s;
        if (h_tslist) h_tslist[i] = f.ts;
    }
    return count;
}

int64_t sdfa_stream_final_frames(int64_t n_samples, int sample_rate, int fps, int win, int hop) {
    if (n_samples < 0 || sample_rate <= 0 || fps <= 0 || win <= 0 || hop <= 0) return sdfa_fail(SDFA_EINVAL, "bad stream_final_frames arguments");
    if (n_samples > 0x1fffffff) return sdfa_fail(SDFA_EINVAL, "frame_index: clips of more than 2^29 - 1 samples are not supported (%lld given)", (long long)n_samples);
    const int64_t sliding = (int64_t)hop * 63 + win;
    // final: e_k < n, one sample past the window (include/sdfa_stream.h); none while n - 1 < sliding
    const int64_t m = n_samples - 1;
    if (m < sliding) return 0;
    // e_k does not decrease with k (a float32 rounding of an increasing value): the largest k with e_k <= n, by bisection
    auto end_of = [&](int64_t k) { return frame_pos((double)k - 1.0, sample_rate, fps, sliding, 0).e; };
    int64_t lo = 0, hi = m * fps / sample_rate + 3;                // e_lo <= m < e_hi
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        (end_of(mid) <= m ? lo : hi) = mid;
    }
    return lo + 1;
}

int sdfa_stream_ring_append(float *d_rings, int r, int32_t n_rings, const int64_t *d_seg, int32_t n_seg, const float *d_src,
                            int64_t n_src, void *stream) {
    if (n_seg == 0) return SDFA_OK;
    if (!d_rings || !d_seg || !d_src || n_seg < 0 || n_rings <= 0 || n_src < 0 || r < 1 || r > 28)
        return sdfa_fail(SDFA_EINVAL, "stream_ring_append: null pointer or bad count");
    HIP_TRY(sdfa_launch_ring_append(d_rings, r, n_rings, d_seg, n_seg, d_src, n_src, (hipStream_t)stream));
    return SDFA_OK;
}

int sdfa_mel_frontend_ring(const float *d_rings, int r, int32_t n_rings, const int64_t *d_view_ring, const int64_t *d_view_hi,
                           int32_t n_views, const int32_t *d_frame_view, const int64_t *d_frame_start, int64_t n_frames,
                           int sample_rate, float *d_audio_feat, void *d_workspace, int64_t workspace_bytes, void *stream) {
    if (n_frames == 0) return SDFA_OK;
    if (!d_rings || !d_view_ring || !d_view_hi || !d_frame_view || !d_frame_start || !d_audio_feat || !d_workspace || n_rings <= 0 ||
        n_views <= 0 || n_frames < 0)
        return sdfa_fail(SDFA_EINVAL, "mel_frontend_ring: null pointer or bad count");
    if (((uintptr_t)d_workspace | (uintptr_t)d_audio_feat) & 15) return sdfa_fail(SDFA_EINVAL, "mel_frontend_ring: pointers must be 16-byte aligned");
    // the offline call's column transform at 16 kHz is column_mel_r8 in every form but "mel_fft_radix4" (the radix-4 transform of rounds
    // 2-3, which rounds differently): with that switch on, a live frame could not equal the offline frame, so the call is refused
    if (g_sdfa_mel_fft_radix4 && (int)(0.064 * sample_rate) == 1024)
        return sdfa_fail(SDFA_EINVAL, "mel_frontend_ring: the \"mel_fft_radix4\" option is on; live frames are bit-equal to the default offline transform only");
    const FeWs w = fe_layout(n_frames);
    if (workspace_bytes < w.total)
        return sdfa_fail(SDFA_ENOSPACE, "mel_frontend_ring: workspace of %lld bytes, %lld needed for %lld frames", (long long)workspace_bytes,
                    (long long)w.total, (long long)n_frames);
    if (w.Mc >= (int64_t)1 << 31) return sdfa_fail(SDFA_EINVAL, "mel_frontend_ring: too many frames in one call");
    FrontendConsts c;
    if (int rc = frontend_consts(sample_rate, c)) return rc;
    if (r < 1 || r > 28 || ((int64_t)1 << r) < (int64_t)c.hop * 63 + c.win)
        return sdfa_fail(SDFA_EINVAL, "mel_frontend_ring: rings of 2^%d samples cannot hold a window of %d samples (r <= 28)", r, c.hop * 63 + c.win);
    hipStream_t s = (hipStream_t)stream;
    int32_t *sh = reinterpret_cast<int32_t *>(d_workspace);
    ShareArgs sa{};
    sa.frame_clip = d_frame_view; sa.frame_start = d_frame_start; sa.hop = c.hop;
    sa.t_lo = 1; sa.t_hi = 63;
    sa.frame_major = 1;
    sa.N = n_frames; sa.Nc = w.Nc; sa.Mc = w.Mc;
    sdfa_share_carve(sa, sh);      // only prev / shift are used
    HIP_TRY(hipMemsetAsync(sh + 8, 0, sizeof(int32_t), s));      // the status word, as sdfa_mel_frontend_gather
    HIP_TRY(sdfa_launch_share_prev(sa, s));
    HIP_TRY(sdfa_launch_mel_ring(c, d_rings, r, n_rings, d_view_ring, d_view_hi, d_frame_view, d_frame_start, sa.prev, sa.shift, n_frames,
                                 g_sdfa_frontend_stream_block, g_sdfa_frontend_stream_slots, g_sdfa_frontend_stream_phases ? 0 : 1,
                                 g_sdfa_frontend_stream_spin_max, sh + 8, d_audio_feat, s));
    return SDFA_OK;
}

}  // extern "C"
