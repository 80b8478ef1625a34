/* A plain C caller (hipMalloc, no Python) that separates a track through the C ABI of include/wun.h: a small stereo context
 * model with a fixed parameter pattern, a synthetic track, wun_separate_track, the estimates written to argv[1] as raw
 * float32 [S, n_frames, C].  Built and run by tests/test_gpu_track.py, which compares the file with the Python path:
 *   hipcc -x c -D__HIP_PLATFORM_AMD__ -Iinclude tests/track_smoke.c -Lwave-u-net_amd -lwun -o track_smoke
 * Reference surface: the hop loop of Evaluate.predict_track (Evaluate.py:113-143) around get_output.
 * Every hip* and wun_* return value is checked; the first failure ends the program with a non-zero status. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <hip/hip_runtime_api.h>
#include "wun.h"

#define HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    fprintf(stderr, "track_smoke: FAILED %s: %s\n", #call, hipGetErrorString(e_)); return 2; } } while (0)
#define WUN(call) do { int r_ = (int)(call); if (r_ != WUN_OK) { \
    fprintf(stderr, "track_smoke: FAILED %s: status %d (%s)\n", #call, r_, wun_last_error()); return 3; } } while (0)

/* element i of a pattern in (-0.125, 0.125): 16 bits of a multiplicative hash, every step exact in float32
 * (tests/test_gpu_track.py computes the same floats with numpy) */
static float pattern(uint32_t i, uint32_t mul) {
    const uint32_t h = ((uint32_t)(i * mul) >> 8) & 0xFFFFu;
    return ((float)h / 65536.0f - 0.5f) * 0.25f;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: track_smoke <output file>\n"); return 1; }
    wun_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.num_layers = 3; cfg.num_initial_filters = 8; cfg.filter_size = 15; cfg.merge_filter_size = 5;
    cfg.input_filter_size = 15; cfg.output_filter_size = 1; cfg.context = 1; cfg.num_sources = 2; cfg.num_channels = 2;
    const int64_t batch = 3, C = cfg.num_channels, S = cfg.num_sources;
    int64_t tin = 0, tout = 0;
    WUN(wun_get_padding(&cfg, 40, &tin, &tout));
    wun_plan* plan = NULL;
    WUN(wun_plan_create(&cfg, batch, tin, &plan));
    wun_plan_info info;
    WUN(wun_plan_query(plan, &info));

    const int64_t n_frames = 7 * tout + 17;                   /* 8 hops: chunks of 3, 3, 2; the last hop re-aligned */
    const int64_t pad = (tin - tout) / 2, track_frames = n_frames + 2 * pad;
    if (wun_separate_positions(tout, n_frames, NULL, 0) != 8) { fprintf(stderr, "track_smoke: FAILED hop count\n"); return 4; }

    float* h_params = (float*)malloc(sizeof(float) * (size_t)info.arena_floats);
    float* h_track = (float*)calloc((size_t)(track_frames * C), sizeof(float));
    float* h_preds = (float*)malloc(sizeof(float) * (size_t)(S * n_frames * C));
    if (!h_params || !h_track || !h_preds) { fprintf(stderr, "track_smoke: FAILED malloc\n"); return 4; }
    for (int64_t i = 0; i < info.arena_floats; ++i) h_params[i] = pattern((uint32_t)i, 2654435761u);
    for (int64_t i = 0; i < n_frames * C; ++i) h_track[pad * C + i] = 4.0f * pattern((uint32_t)i, 40503u);

    float *params = NULL, *track = NULL, *ws = NULL, *outs = NULL, *preds = NULL;
    HIP(hipMalloc((void**)&params, sizeof(float) * (size_t)info.arena_floats));
    HIP(hipMalloc((void**)&track, sizeof(float) * (size_t)(track_frames * C)));
    HIP(hipMalloc((void**)&ws, sizeof(float) * (size_t)info.workspace_floats));
    HIP(hipMalloc((void**)&outs, sizeof(float) * (size_t)(S * batch * tout * C)));
    HIP(hipMalloc((void**)&preds, sizeof(float) * (size_t)(S * n_frames * C)));
    HIP(hipMemcpy(params, h_params, sizeof(float) * (size_t)info.arena_floats, hipMemcpyHostToDevice));
    HIP(hipMemcpy(track, h_track, sizeof(float) * (size_t)(track_frames * C), hipMemcpyHostToDevice));
    HIP(hipMemset(preds, 0xFF, sizeof(float) * (size_t)(S * n_frames * C)));      /* NaN: every frame must be written */

    WUN(wun_separate_track(plan, params, track, n_frames, ws, outs, preds, NULL));
    HIP(hipStreamSynchronize(NULL));
    HIP(hipMemcpy(h_preds, preds, sizeof(float) * (size_t)(S * n_frames * C), hipMemcpyDeviceToHost));

    FILE* f = fopen(argv[1], "wb");
    if (!f) { fprintf(stderr, "track_smoke: FAILED fopen %s\n", argv[1]); return 5; }
    const size_t n = (size_t)(S * n_frames * C);
    if (fwrite(h_preds, sizeof(float), n, f) != n || fclose(f) != 0) { fprintf(stderr, "track_smoke: FAILED fwrite\n"); return 5; }

    HIP(hipFree(preds)); HIP(hipFree(outs)); HIP(hipFree(ws)); HIP(hipFree(track)); HIP(hipFree(params));
    wun_plan_destroy(plan);
    free(h_preds); free(h_track); free(h_params);
    printf("track_smoke: ok (%lld frames, %lld hops of %lld, %lld sources, %s)\n", (long long)n_frames, 8LL, (long long)tout,
           (long long)S, wun_version());
    return 0;
}
