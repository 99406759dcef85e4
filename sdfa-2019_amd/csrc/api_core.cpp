// C ABI of libsdfa_hip.so (include/sdfa_hip.h): the error string, ABI versions and the A/B option table.
#include "../../include/sdfa_stream.h"
#include "host.h"

#include <climits>
#include <cstdio>
#include <cstring>
#include <string>

static thread_local std::string g_err;

int sdfa_failv(int code, const char *fmt, va_list ap) {
    char buf[512];
    vsnprintf(buf, sizeof buf, fmt, ap);
    g_err = buf;
    return code;
}

int sdfa_fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    sdfa_failv(code, fmt, ap);
    va_end(ap);
    return code;
}

// A/B tuning switches: THREAD-LOCAL, so that a thread that flips one for an experiment cannot change what concurrent
// callers on other threads launch (the header promises thread-safe concurrent use of the forward calls).  An option is
// its variable here, its row in the table of sdfa_debug_set_option below and its row in the comment table next to that
// function's declaration in include/sdfa_hip.h (tests/test_abi_cpu.py holds the two tables against each other).
thread_local int g_sdfa_mel_fft_radix4 = 0;     // "mel_fft_radix4" option (read by frontend.hip)
thread_local int g_sdfa_gather_plain_order = 0; // "gather_plain_order" option (read by frontend.hip)
thread_local int g_sdfa_frontend_two_kernel = 0;    // "frontend_two_kernel": 1 = share map + mel_columns + gather_features (rounds 2-4) instead of the spectral stream
thread_local int g_sdfa_frontend_stream_block = 0; // "frontend_stream_block" / "frontend_stream_slots": segment geometry of the spectral stream (0 = default)
thread_local int g_sdfa_frontend_stream_slots = 0;
thread_local int g_sdfa_frontend_stream_spin_max = 0; // "frontend_stream_spin_max" (tests): bound of the producer / consumer hand-off waits in polls (0 = the kernel's 4 M); 1 makes them expire, the repair pass redoes the call in the barrier form
thread_local int g_sdfa_frontend_stream_phases = 0; // "frontend_stream_phases": 1 = the stream kernel's workgroups alternate between transforming and emitting (a barrier pair per phase) instead of producer / consumer waves
thread_local int g_sdfa_frontend_t_major = 0;   // "frontend_t_major" option: the front end's distinct columns numbered time-step-major (rounds 2-3)
extern thread_local int g_sdfa_gemm_variant;  // defined in gemm.hip
thread_local int g_sdfa_freq_lstm_shape = 0;
thread_local int g_sdfa_pca_lds = 0;
thread_local int g_sdfa_pca_fp32 = 0;     // "pca_fp32": 1 = the dgrad PCA expansion stays on the fp32 kernel in SDFA_PREC_BF16X3 (A/B)
thread_local int g_sdfa_conv_fp32 = 0;    // "conv_fp32": 1 = the conv stack stays on the fp32 kernel in the mixed-precision modes (A/B)
thread_local int g_sdfa_time_lstm_split = 0;
thread_local int g_sdfa_time_lstm_fuse_x = 0;   // "time_lstm_fuse_x": layer 1 of the BiLSTM contracts its input projection inside the recurrence: 0 = by size, 1 = never, 2 / 3 = always (32- / 64-frame tiles)
thread_local int g_sdfa_time_lstm_handoff = 0;
thread_local int g_sdfa_time_lstm_timeout_us = 0;
thread_local int g_sdfa_share_gx0_off = 0;
thread_local int g_sdfa_encoder_dedup_off = 0; // "encoder_dedup_off": 1 = sdfa_encoder_forward evaluates every column (no scan of audio_feat for identical columns)
thread_local int g_sdfa_share_hash_bits = 0;  // "share_hash_bits" (tests): the encoder's column scan groups by the low n bits of its 64-bit hash only (0 = all of them), so that hashes collide and the full compare decides
thread_local int g_sdfa_freq_proj_tail = 0;   // "freq_proj_tail": the shared-column frequency projection's last partial round of gemm_fat_kernel in fine tiles (gemm_tail.hip): 0 = where the device-side rule says it pays, 1 = never, 2 = always
thread_local int g_sdfa_attn_unfused = 0;  // "attn_unfused": 1 = the bf16 attention modes keep the three-GEMM + attn_kernel form of round 5 (A/B)

extern "C" {

int sdfa_abi_version(void) { return SDFA_ABI_VERSION; }
int sdfa_stream_abi_version(void) { return SDFA_STREAM_ABI_VERSION; }
const char *sdfa_last_error(void) { return g_err.c_str(); }

int sdfa_debug_set_option(const char *name, int value) {
    struct Option { const char *name; int *var; int lo = INT_MIN, hi = INT_MAX; const char *accepts = nullptr; };
    // thread_local: the address of a thread's copy of a switch is not a constant, so each thread fills its table on its first call
    thread_local const Option options[] = {
        {"attn_unfused", &g_sdfa_attn_unfused},
        {"share_gx0_off", &g_sdfa_share_gx0_off},
        {"encoder_dedup_off", &g_sdfa_encoder_dedup_off},
        {"share_hash_bits", &g_sdfa_share_hash_bits, 0, 32, "0 (the whole hash) or 1..32 low bits"},
        {"freq_proj_tail", &g_sdfa_freq_proj_tail, 0, 2, "0 (rule), 1 (never) or 2 (always)"},
        {"frontend_two_kernel", &g_sdfa_frontend_two_kernel},
        {"frontend_stream_phases", &g_sdfa_frontend_stream_phases},
        {"frontend_stream_spin_max", &g_sdfa_frontend_stream_spin_max, 0, INT_MAX, "0 (default) or a positive poll count"},
        {"frontend_stream_block", &g_sdfa_frontend_stream_block, 0, 256, "0 (default) or 1..256 frames"},
        {"frontend_stream_slots", &g_sdfa_frontend_stream_slots, 0, 256, "0 (default) or 1..256 workgroups per block"},
        {"gather_plain_order", &g_sdfa_gather_plain_order},
        {"mel_fft_radix4", &g_sdfa_mel_fft_radix4},
        {"frontend_t_major", &g_sdfa_frontend_t_major},
        {"time_lstm_timeout_us", &g_sdfa_time_lstm_timeout_us},
        {"time_lstm_handoff", &g_sdfa_time_lstm_handoff},
        {"time_lstm_split", &g_sdfa_time_lstm_split},
        {"time_lstm_fuse_x", &g_sdfa_time_lstm_fuse_x, 0, 3, "0 (rule), 1 (never), 2 or 3 (always, 32- / 64-frame tiles)"},
        {"gemm_variant", &g_sdfa_gemm_variant},
        {"freq_lstm_shape", &g_sdfa_freq_lstm_shape},
        {"pca_lds", &g_sdfa_pca_lds},
        {"conv_fp32", &g_sdfa_conv_fp32},
        {"pca_fp32", &g_sdfa_pca_fp32},
    };
    for (const Option &o : options)
        if (name && !strcmp(name, o.name)) {
            if (value < o.lo || value > o.hi) return sdfa_fail(SDFA_EINVAL, "%s: %s", o.name, o.accepts);
            *o.var = value;
            return SDFA_OK;
        }
    return sdfa_fail(SDFA_EINVAL, "unknown option '%s'", name ? name : "(null)");
}

}  // extern "C"
