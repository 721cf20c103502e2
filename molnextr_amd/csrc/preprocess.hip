// preprocess.hip — the transform in front of the encoder, on device:
//   CropWhite(pad) [-> PadToSquare] -> Resize(S,S, bilinear) -> ToGray -> Normalize(ImageNet) -> CHW fp32
//   reference MolNexTR/dataset.py:158-185 (augment=False), MolNexTR/data_aug.py:98-143, MolNexTR/model.py:104.
// Integer / byte work, HBM-trivial (one pass over the page for the bounding box, then 4 taps per output pixel).
// It computes bit for bit what molnextr_amd/preprocess.py computes (the host restatement of albumentations 1.1.0 /
// OpenCV semantics). Pinned: both lie within 2 grey levels of exact half-pixel-centre bilinear interpolation in float64
// (tests/prep_ref.py, anchored on torch.nn.functional.interpolate; tests/test_gpu_prep_ref.py holds these kernels to it).
// Not pinned: OpenCV's exact rounding inside that bound, see molnextr_amd/preprocess.py.
#include "common.h"
#include "kernels.h"

namespace mnx {

// bbox = {min row, max row, min col, max col} of pixels that differ from white in any channel; max = -1 when blank
__global__ void prep_bbox_init_kernel(int* bbox, int H, int W) {
    if (threadIdx.x == 0) { bbox[0] = H; bbox[1] = -1; bbox[2] = W; bbox[3] = -1; }
}

__global__ __launch_bounds__(256) void prep_bbox_kernel(const uint8_t* __restrict__ rgb, int H, int W, int* bbox) {
    __shared__ int s_min[4], s_max[4];
    const int y = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* row = rgb + (size_t)y * W * 3;
    int mn = W, mx = -1;
    for (int x = tid; x < W; x += 256) {
        const bool ink = row[3 * x] != 255 || row[3 * x + 1] != 255 || row[3 * x + 2] != 255;
        if (ink) { mn = min(mn, x); mx = max(mx, x); }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = min(mn, __shfl_xor(mn, o, 64));
        mx = max(mx, __shfl_xor(mx, o, 64));
    }
    if (lane == 0) { s_min[wave] = mn; s_max[wave] = mx; }
    __syncthreads();
    if (tid == 0) {
        mn = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
        mx = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
        if (mx >= 0) {
            atomicMin(&bbox[0], y); atomicMax(&bbox[1], y);
            atomicMin(&bbox[2], mn); atomicMax(&bbox[3], mx);
        }
    }
}

// cv2.resize(INTER_LINEAR) tap for 8-bit images: source index, neighbour, and the two 11-bit weights
__device__ __forceinline__ void linear_tap(int d, int src, int dst, int& i0, int& i1, int& w0, int& w1) {
    const double scale = 1.0 / ((double)dst / (double)src);
    // separate multiply and subtract (no fused multiply-add): the host restatement rounds twice
    const float fx = (float)__dsub_rn(__dmul_rn((double)d + 0.5, scale), 0.5);
    int sx = (int)floorf(fx);
    float frac = fx - (float)sx;
    if (sx < 0) { frac = 0.f; sx = 0; }
    if (sx >= src - 1) { frac = 0.f; sx = src - 1; }
    w0 = (int)rintf((1.0f - frac) * 2048.0f);
    w1 = (int)rintf(frac * 2048.0f);
    i0 = sx;
    i1 = min(sx + 1, src - 1);
}

struct PrepArgs {
    const uint8_t* rgb;
    const int* bbox;
    int* crop_out;       // or null: {crop_top, crop_bottom, crop_left, crop_right} as CropWhite.update_params reports
    float* out;          // [3, S, S]
    int H, W, pad, S, square;
    float mean255[3], inv[3];
};

__global__ __launch_bounds__(256) void prep_resize_kernel(PrepArgs a) {
    constexpr bool GRAY8 = false;
#include "prep_resize_body.inc"
}

// ---- all pages of one mnx_preprocess_batch call: three launches whatever n ----------------------------------------------
// The pages are ragged and their table lives on the device (the host never reads it), so the box kernel runs a
// (row, page) grid of max_height x n workgroups in which a workgroup whose row lies beyond its page leaves at once: a
// flattened row index would need the prefix sums of the heights, i.e. a host pass over the table or a device scan in front,
// for workgroups that cost nothing when they exit on their first compare. Every address into the arena is 64-bit.
__global__ __launch_bounds__(256) void prep_bbox_init_batch_kernel(const mnx_page* __restrict__ pages, int n, int* bbox) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) { bbox[4 * i] = pages[i].height; bbox[4 * i + 1] = -1; bbox[4 * i + 2] = pages[i].width; bbox[4 * i + 3] = -1; }
}

__global__ __launch_bounds__(256) void prep_bbox_batch_kernel(const uint8_t* __restrict__ arena,
                                                              const mnx_page* __restrict__ pages, int* bbox) {
    __shared__ int s_min[4], s_max[4];
    const mnx_page pg = pages[blockIdx.y];
    const int y = blockIdx.x, W = pg.width, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (y >= pg.height) return;       // uniform over the workgroup
    const uint8_t* row = arena + (size_t)pg.offset + (size_t)y * W * 3;
    int mn = W, mx = -1;
    for (int x = tid; x < W; x += 256) {
        const bool ink = row[3 * x] != 255 || row[3 * x + 1] != 255 || row[3 * x + 2] != 255;
        if (ink) { mn = min(mn, x); mx = max(mx, x); }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = min(mn, __shfl_xor(mn, o, 64));
        mx = max(mx, __shfl_xor(mx, o, 64));
    }
    if (lane == 0) { s_min[wave] = mn; s_max[wave] = mx; }
    __syncthreads();
    if (tid == 0) {
        int* bb = bbox + 4 * blockIdx.y;
        mn = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
        mx = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
        if (mx >= 0) {
            atomicMin(&bb[0], y); atomicMax(&bb[1], y);
            atomicMin(&bb[2], mn); atomicMax(&bb[3], mx);
        }
    }
}

struct PrepBatchArgs {
    const uint8_t* arena;
    const mnx_page* pages;
    const int* bbox;     // [n][4]
    int* crops;          // [n][4] or null
    void* out;           // GRAY8: uint8 [n, S, S]; otherwise fp32 [n, 3, S, S]
    int pad, S, square;
    NormConsts nc;
};

template <bool GRAY8>
__global__ __launch_bounds__(256) void prep_resize_batch_kernel(PrepBatchArgs b) {
    const size_t i = blockIdx.z;
    const mnx_page pg = b.pages[i];
    const size_t img = (size_t)b.S * b.S;
    PrepArgs a;
    a.rgb = b.arena + (size_t)pg.offset;
    a.bbox = b.bbox + 4 * i;
    a.crop_out = b.crops ? b.crops + 4 * i : nullptr;
    a.out = GRAY8 ? (float*)((uint8_t*)b.out + i * img) : (float*)b.out + i * 3 * img;
    a.H = pg.height; a.W = pg.width; a.pad = b.pad; a.S = b.S; a.square = b.square;
#pragma unroll
    for (int c = 0; c < 3; ++c) { a.mean255[c] = b.nc.mean255[c]; a.inv[c] = b.nc.inv[c]; }
#include "prep_resize_body.inc"
}

NormConsts norm_consts() {
    NormConsts k;
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};   // IMAGENET_DEFAULT_MEAN / STD
    for (int c = 0; c < 3; ++c) {
        volatile float m = mean[c] * 255.0f, d = sd[c] * 255.0f;   // fp32 products, as numpy computes them
        k.mean255[c] = m;
        k.inv[c] = 1.0f / d;
    }
    return k;
}

hipError_t launch_preprocess(const uint8_t* rgb, int H, int W, int pad, int square, int S, int* bbox, int* crop_out,
                             float* out, hipStream_t s) {
    hipLaunchKernelGGL(prep_bbox_init_kernel, dim3(1), dim3(64), 0, s, bbox, H, W);
    hipLaunchKernelGGL(prep_bbox_kernel, dim3(H), dim3(256), 0, s, rgb, H, W, bbox);
    PrepArgs a;
    a.rgb = rgb; a.bbox = bbox; a.crop_out = crop_out; a.out = out; a.H = H; a.W = W; a.pad = pad; a.S = S; a.square = square;
    const NormConsts k = norm_consts();
    for (int c = 0; c < 3; ++c) { a.mean255[c] = k.mean255[c]; a.inv[c] = k.inv[c]; }
    hipLaunchKernelGGL(prep_resize_kernel, dim3((S + 15) / 16, (S + 15) / 16), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_preprocess_batch(const uint8_t* arena, const mnx_page* pages, int n, int max_height, int pad, int square,
                                   int S, int* bbox, int* crops, void* out, bool gray8, hipStream_t s) {
    if (n < 1 || n > 65535 || max_height < 1) return hipErrorInvalidValue;      // grid.y / grid.z carry the page
    hipLaunchKernelGGL(prep_bbox_init_batch_kernel, dim3((n + 255) / 256), dim3(256), 0, s, pages, n, bbox);
    hipLaunchKernelGGL(prep_bbox_batch_kernel, dim3(max_height, n), dim3(256), 0, s, arena, pages, bbox);
    PrepBatchArgs a;
    a.arena = arena; a.pages = pages; a.bbox = bbox; a.crops = crops; a.out = out; a.pad = pad; a.S = S; a.square = square;
    a.nc = norm_consts();
    const dim3 grid((S + 15) / 16, (S + 15) / 16, n);
    if (gray8) hipLaunchKernelGGL(prep_resize_batch_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(prep_resize_batch_kernel<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace mnx
