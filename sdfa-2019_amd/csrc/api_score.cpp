// Host side of the validation losses (include/sdfa_score.h): the refusals, the workspace layout and
// the launches of score.hip.  Nothing here copies or synchronises.
#include "host.h"
#include "score.h"

namespace {

struct Layout {
    int64_t first, part, total, nslab;      // byte offsets
};

int check_shape(const char *who, int64_t F, int64_t W, int layout, Layout *l) {
    if (layout != SDFA_SCORE_LAYOUT_DGRAD && layout != SDFA_SCORE_LAYOUT_PLAIN) return sdfa_fail(SDFA_EINVAL, "%s: unknown layout %d", who, layout);
    if (F < 2 || F > 65535ll * SDFA_SCORE_RUN) return sdfa_fail(SDFA_EINVAL, "%s: %lld frames outside 2 .. %lld", who, (long long)F, 65535ll * SDFA_SCORE_RUN);
    if (W < 1 || W > (1ll << 30)) return sdfa_fail(SDFA_EINVAL, "%s: row width %lld outside 1 .. 2^30", who, (long long)W);
    if (layout == SDFA_SCORE_LAYOUT_DGRAD && W % 9 != 0) return sdfa_fail(SDFA_EINVAL, "%s: a dgrad row of %lld values is no multiple of 9", who, (long long)W);
    l->nslab = (W + SDFA_SCORE_COLS - 1) / SDFA_SCORE_COLS;
    l->first = 0;
    l->part = round_up(F, 256);
    l->total = l->part + round_up(F * l->nslab * SDFA_SCORE_PARTS * 4 * 8, 256);
    return SDFA_OK;
}

}  // namespace

extern "C" {

int sdfa_score_abi_version(void) { return SDFA_SCORE_ABI_VERSION; }

int64_t sdfa_score_workspace_bytes(int64_t F, int64_t W, int layout) {
    Layout l;
    const int rc = check_shape("score_workspace_bytes", F, W, layout, &l);
    return rc < 0 ? rc : l.total;
}

int sdfa_score_rows(const float *d_pred, int64_t F, int64_t W, int layout, const float *d_track, int64_t n_track, const int64_t *d_src,
                    const float *d_w, const int64_t *clip_frame_off, int64_t n_clips, double *d_out, void *d_ws, int64_t ws_bytes,
                    void *stream) {
    Layout l;
    const int rc = check_shape("score_rows", F, W, layout, &l);
    if (rc < 0) return rc;
    if (!d_pred || !d_track || !d_src || !d_w || !clip_frame_off || !d_out || !d_ws) return sdfa_fail(SDFA_EINVAL, "score_rows: null pointer");
    if (n_track < 1) return sdfa_fail(SDFA_EINVAL, "score_rows: a track of %lld rows", (long long)n_track);
    if (n_clips < 1 || clip_frame_off[0] != 0 || clip_frame_off[n_clips] != F)
        return sdfa_fail(SDFA_EINVAL, "score_rows: the offsets of %lld clips do not run from 0 to %lld", (long long)n_clips, (long long)F);
    for (int64_t c = 0; c < n_clips; ++c)
        if (clip_frame_off[c + 1] - clip_frame_off[c] < 2 || clip_frame_off[c + 1] > F)
            return sdfa_fail(SDFA_EINVAL, "score_rows: clip %lld has %lld frames, the motion loss needs at least 2", (long long)c,
                             (long long)(clip_frame_off[c + 1] - clip_frame_off[c]));
    if (ws_bytes < l.total) return sdfa_fail(SDFA_EINVAL, "score_rows: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)l.total);
    if ((uintptr_t)d_ws % 256 != 0) return sdfa_fail(SDFA_EINVAL, "score_rows: workspace not 256-byte aligned");

    hipStream_t st = (hipStream_t)stream;
    unsigned char *first = (unsigned char *)d_ws + l.first;
    HIP_TRY(hipMemsetAsync(first, 0, (size_t)F, st));
    ScoreMarks m;
    for (int64_t c = 0; c < n_clips; c += SCORE_MARKS) {
        m.n = (int)(n_clips - c < SCORE_MARKS ? n_clips - c : SCORE_MARKS);
        for (int i = 0; i < m.n; ++i) m.off[i] = clip_frame_off[c + i];
        HIP_TRY(score_mark(m, first, st));
    }
    ScoreArgs a;
    a.pred = d_pred;
    a.track = d_track;
    a.src = d_src;
    a.w = d_w;
    a.first = first;
    a.part = (double *)((char *)d_ws + l.part);
    a.out = d_out;
    a.F = F;
    a.W = W;
    a.n_track = n_track;
    a.nslab = l.nslab;
    HIP_TRY(score_launch(a, layout, st));
    return SDFA_OK;
}

}  // extern "C"
