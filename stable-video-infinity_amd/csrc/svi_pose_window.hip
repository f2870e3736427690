// svi_pose_window.hip — the clip pose window of the dance stream, cut on the device, and the host statement of its rule (svi_pose_window,
// svi_pose_window_plan).  A source file of its own: it shares no device code with the profiled kernels, whose committed counter summaries are keyed to
// the hashes of their sources.
//
// What the reference's script does between two clips on the host (test_svi_dance.py:215-227, 281-288 around utils/image_process.py:134-170): a rolling
// window over the whole pose video that carries the last m poses of the previous window and reads on from a cursor that wraps, every frame resized
// with nearest-neighbour to the clip size, padded to the centre and converted to float.  The rule is stated in full at svi_pose_window in the public
// header; the two index functions below ARE the rule, for the kernel and for svi_pose_window_plan.
// pose u8 [N, h, w, 3] -> out f32 [3, F, H, W].  A lane owns four neighbouring columns of one (frame, row) in all three channels: the three bytes of a
// source pixel are neighbours, so they are read together, and every channel plane gets one 16-byte store — a wave's stores are 1 KB runs, its reads walk
// one source row (two at a row's end) in step with the nearest map.  The source frame depends on blockIdx alone.
#include <math.h>

#include "svi_common.h"

namespace {
struct PoseWindow { int N, h, w, H, W, F, m, k; int nh, nw, pad_top, pad_left; float rs_h, rs_w; };

__host__ __device__ inline long long pose_window_frame(int F, int m, long long k, int i, int N) {
    while (k > 0 && i < m) { i += F - m; --k; }                 // a carried motion pose: the same pose of the window before (at most m rounds: i grows)
    const long long g = k == 0 ? (long long)i : (long long)(F - 1) + (k - 1) * (long long)(F - m) + (i - m);
    return g % N;
}
__host__ __device__ inline int pose_window_src(int o, int pad, int n, int size, float rs) {
    const int t = o - pad;
    if (t < 0 || t >= n) return -1;                             // padding
    const int s = (int)floorf((float)t * rs);
    return s < size - 1 ? s : size - 1;
}

// the scalars' checks and the sizes, for both entry points (`who` names the caller in the message)
svi_status pose_window_geometry(const char* who, int N, int h, int w, int H, int W, int F, int m, int k, PoseWindow* out) {
    SVI_REQUIRE(N >= 1, "%s: N = %d pose frames (at least one)", who, N);
    SVI_REQUIRE(F >= 2, "%s: F = %d frames per clip (at least two)", who, F);
    SVI_REQUIRE(m >= 1 && m < F, "%s: m = %d motion frames must be in 1 .. F - 1 = %d", who, m, F - 1);
    SVI_REQUIRE(k >= 0, "%s: k = %d is negative", who, k);
    SVI_REQUIRE(h >= 1 && w >= 1, "%s: source size h = %d, w = %d (at least 1 x 1)", who, h, w);
    SVI_REQUIRE(H >= 16 && W >= 16, "%s: clip size H = %d, W = %d (at least 16 x 16)", who, H, W);
    const double hs = (double)H / (double)h, ws = (double)W / (double)w;
    const double s = hs < ws ? hs : ws;
    PoseWindow p{N, h, w, H, W, F, m, k, (int)((double)h * s), (int)((double)w * s), 0, 0, 0.0f, 0.0f};
    SVI_REQUIRE(p.nh >= 1 && p.nw >= 1, "%s: %d x %d scaled into %d x %d is nh = %d, nw = %d (at least 1 x 1)", who, h, w, H, W, p.nh, p.nw);
    p.pad_top = (H - p.nh) / 2;
    p.pad_left = (W - p.nw) / 2;
    p.rs_h = (float)h / (float)p.nh;
    p.rs_w = (float)w / (float)p.nw;
    *out = p;
    return SVI_OK;
}

template <bool VEC>
__global__ __launch_bounds__(256) void pose_window_kernel(const unsigned char* __restrict__ pose, float* __restrict__ out, PoseWindow p, int Wq) {
    const int i = blockIdx.y;                                   // window frame
    const int idx = blockIdx.x * 256 + threadIdx.x;             // over H rows x Wq column quads
    if (idx >= p.H * Wq) return;
    const int y = idx / Wq, x0 = (idx - y * Wq) * 4;
    const int sy = pose_window_src(y, p.pad_top, p.nh, p.h, p.rs_h);
    float v[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[c][j] = 0.0f;
    if (sy >= 0) {
        const unsigned char* row = pose + ((size_t)pose_window_frame(p.F, p.m, p.k, i, p.N) * p.h + sy) * ((size_t)p.w * 3);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int sx = x0 + j < p.W ? pose_window_src(x0 + j, p.pad_left, p.nw, p.w, p.rs_w) : -1;
            if (sx >= 0) {
                const unsigned char* px = row + (size_t)sx * 3;
                v[0][j] = (float)px[0]; v[1][j] = (float)px[1]; v[2][j] = (float)px[2];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* o = out + (((size_t)c * p.F + i) * p.H + y) * p.W + x0;
        if constexpr (VEC) *reinterpret_cast<f32x4*>(o) = f32x4{v[c][0], v[c][1], v[c][2], v[c][3]};
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < p.W) o[j] = v[c][j];
        }
    }
}

svi_status launch_pose_window(const unsigned char* pose, float* out, const PoseWindow& p, hipStream_t st) {
    SVI_REQUIRE(p.F <= 65535, "svi_pose_window: F = %d frames per clip (at most 65535)", p.F);
    SVI_REQUIRE((long long)p.H * p.W < (1LL << 31) - 4096, "svi_pose_window: a %d x %d frame passes the launch's 2^31 elements", p.H, p.W);
    SVI_REQUIRE(((uintptr_t)out & 3) == 0, "svi_pose_window: out must be 4-byte aligned");
    const int Wq = (p.W + 3) / 4;
    const dim3 grid((unsigned)(((long long)p.H * Wq + 255) / 256), (unsigned)p.F), block(256);
    if (p.W % 4 == 0 && ((uintptr_t)out & 15) == 0) hipLaunchKernelGGL(pose_window_kernel<true>, grid, block, 0, st, pose, out, p, Wq);
    else hipLaunchKernelGGL(pose_window_kernel<false>, grid, block, 0, st, pose, out, p, Wq);
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}
}  // namespace

extern "C" svi_status svi_pose_window(const uint8_t* pose, float* out, int32_t N, int32_t h, int32_t w, int32_t H, int32_t W, int32_t F, int32_t m,
                                      int32_t k, svi_stream stream) {
    SVI_REQUIRE(pose, "svi_pose_window: pose is NULL");
    SVI_REQUIRE(out, "svi_pose_window: out is NULL");
    PoseWindow p;
    SVI_TRY(pose_window_geometry("svi_pose_window", N, h, w, H, W, F, m, k, &p));
    if (svi_current_device() < 0) return SVI_ERR_HIP;
    return launch_pose_window(pose, out, p, reinterpret_cast<hipStream_t>(stream));
}

extern "C" svi_status svi_pose_window_plan(int32_t N, int32_t h, int32_t w, int32_t H, int32_t W, int32_t F, int32_t m, int32_t k, int32_t* frame_src,
                                           int32_t* row_src, int32_t* col_src) {
    SVI_REQUIRE(frame_src && row_src && col_src, "svi_pose_window_plan: NULL output");
    PoseWindow p;
    SVI_TRY(pose_window_geometry("svi_pose_window_plan", N, h, w, H, W, F, m, k, &p));
    for (int i = 0; i < p.F; ++i) frame_src[i] = (int32_t)pose_window_frame(p.F, p.m, p.k, i, p.N);
    for (int y = 0; y < p.H; ++y) row_src[y] = pose_window_src(y, p.pad_top, p.nh, p.h, p.rs_h);
    for (int x = 0; x < p.W; ++x) col_src[x] = pose_window_src(x, p.pad_left, p.nw, p.w, p.rs_w);
    return SVI_OK;
}
