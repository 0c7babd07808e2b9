// View preparation of the scene driver (gfx950): one uint8 BGR image -> the network input and the 1/4-scale image.
//
// Replaces the per-view numpy work of eval_pointcloud.load_data (reference eval_pointcloud.py:97-203): cv2.resize by the map's
// adaptive scale (preprocess.scale_image's uint8 path), the centre crop (crop_mvs_input), center_image, and the 1/4 resize of the
// cropped image.  The host computes every tap index and 11-bit weight with preprocess.py's own code (only the rows / columns the
// kernel writes), so the resize is the same integer arithmetic on the same integers: bit for bit scale_image.
#include "common.h"

// taps: (4, n) int32 rows = left index, right index, left weight, right weight (the weights sum to 2048).
// One thread per output pixel, all three channels; `sums` (6 u64: sum x per channel, sum x^2 per channel) is accumulated when
// non-NULL -- per-wavefront shuffles, one LDS pass, 6 integer atomics per workgroup: exact and order-independent.
__global__ __launch_bounds__(256) void prepare_resize_kernel(const uint8_t* __restrict__ src, int h, int w, uint8_t* __restrict__ dst,
                                                             int H, int W, const int* __restrict__ ytap,
                                                             const int* __restrict__ xtap, unsigned long long* __restrict__ sums) {
  __shared__ unsigned int part[4][6];
  const long n = (long)H * W;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  unsigned int v[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  if (i < n) {
    const int oy = (int)(i / W), ox = (int)(i % W);
    // clamped: a tap list that does not belong to this source can give wrong pixels, never an out-of-bounds read
    const int y0 = min(max(ytap[oy], 0), h - 1), y1 = min(max(ytap[H + oy], 0), h - 1);
    const int by0 = ytap[2 * H + oy], by1 = ytap[3 * H + oy];
    const int x0 = min(max(xtap[ox], 0), w - 1), x1 = min(max(xtap[W + ox], 0), w - 1);
    const int ax0 = xtap[2 * W + ox], ax1 = xtap[3 * W + ox];
    const uint8_t* r0 = src + (size_t)y0 * w * 3;
    const uint8_t* r1 = src + (size_t)y1 * w * 3;
    uint8_t* o = dst + (size_t)i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      // preprocess.scale_image: horiz in 8.11 fixed point, >> 4, the two 16-bit-shifted products, (acc + 2) >> 2, clipped
      const int top = ((int)r0[x0 * 3 + c] * ax0 + (int)r0[x1 * 3 + c] * ax1) >> 4;
      const int bot = ((int)r1[x0 * 3 + c] * ax0 + (int)r1[x1 * 3 + c] * ax1) >> 4;
      const int acc = ((by0 * top) >> 16) + ((by1 * bot) >> 16);
      const int q = min(max((acc + 2) >> 2, 0), 255);
      o[c] = (uint8_t)q;
      v[c] = (unsigned int)q;
      v[3 + c] = (unsigned int)(q * q);
    }
  }
  if (sums == nullptr) return;                                  // uniform over the launch
#pragma unroll
  for (int k = 0; k < 6; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) part[wave][k] = v[k];             // <= 256 * 255^2 per workgroup: fits 32 bits
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const unsigned long long s = (unsigned long long)part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] +
                                 part[3][threadIdx.x];
    if (s) atomicAdd(sums + threadIdx.x, s);
  }
}

// y = (x - mu) / (sd + 1e-8f) in float32 (center_image's expression), mu and sd of each channel from the exact integer sums:
// mu = S1 / n and sd = sqrt((n S2 - S1^2) / n^2) in double, each rounded once to float32.  Four elements per thread.
__global__ __launch_bounds__(256) void prepare_center_kernel(const uint8_t* __restrict__ x, long n, const unsigned long long* __restrict__ sums,
                                                             float* __restrict__ y) {
  float mu[3], den[3];
  const double dn = (double)n;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long long s1 = (long long)sums[c], s2 = (long long)sums[3 + c];
    const long long num = (long long)n * s2 - s1 * s1;           // exact: n * sum x^2 <= 255^2 n^2 < 2^63 for n < 1.1e7
    mu[c] = (float)((double)s1 / dn);
    den[c] = (float)sqrt((double)(num < 0 ? 0 : num) / (dn * dn)) + 1e-8f;
  }
  const long total = n * 3;
  const long base = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long e = base + k;
    if (e < total) {
      const int c = (int)(e % 3);
      y[e] = ((float)x[e] - mu[c]) / den[c];
    }
  }
}

extern "C" int atvs_prepare_resize_u8(const unsigned char* src, int h, int w, unsigned char* dst, int H, int W, const int* ytap,
                                      const int* xtap, unsigned long long* sums, atvs_stream_t stream) {
  if (!src || !dst || !ytap || !xtap) return ATVS_ERR_NULL;
  if (h < 1 || w < 1 || H < 1 || W < 1) return ATVS_ERR_SHAPE;
  hipStream_t st = as_stream(stream);
  if (sums && hipMemsetAsync(sums, 0, 6 * sizeof(unsigned long long), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  prepare_resize_kernel<<<cdiv((long)H * W, 256), 256, 0, st>>>(src, h, w, dst, H, W, ytap, xtap, sums);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_prepare_center(const unsigned char* x, long pixels, const unsigned long long* sums, float* y,
                                   atvs_stream_t stream) {
  if (!x || !sums || !y) return ATVS_ERR_NULL;
  if (pixels < 1 || pixels > 11000000L) return ATVS_ERR_SHAPE;
  prepare_center_kernel<<<cdiv(pixels * 3, 1024), 256, 0, as_stream(stream)>>>(x, pixels, sums, y);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}
