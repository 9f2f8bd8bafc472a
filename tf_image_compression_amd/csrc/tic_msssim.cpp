// tic_msssim.cpp — MS-SSIM (Wang et al. 2003, with the choices of tf.image.ssim_multiscale) of
// lists of uint8 image pairs that already lie in HBM, and its C-ABI entries (include/tic.h).
//
// The codec was built for the CLIC challenge (submit/), which ranks by PSNR and MS-SSIM; the
// reference itself only has the dataset PSNR (processing_utils/evaluate.py).  Five scales of
// 11x11 Gaussian moments cost seconds per 4K pair on the host, while both images are on the
// device anyway after encode_images_device / decode_images_device.
//
//   msssim_scale_kernel   one workgroup per 16-row x 64-element output tile of one scale of one
//                         image pair.  An image row is taken as 3*w interleaved elements, so the
//                         three channels are one 1-D row with tap stride 3 and a thread's channel
//                         is fixed by its column.  Both tiles plus the 10-sample halo are staged
//                         in LDS as floats centred on 127.5 (the E[x^2] - mu^2 cancellation on
//                         bright flat areas shrinks with the mean), the horizontal 11-tap pass
//                         writes the five moments E[x] E[y] E[xx] E[yy] E[xy] back to LDS, the
//                         vertical pass reads them column-wise (consecutive lanes on consecutive
//                         banks in every pass), four consecutive output rows per wave so that
//                         their overlapping windows are read once, and forms cs and l*cs per
//                         position in float32.
//                         Sums over positions are float64: per thread, then a wave shuffle, then
//                         the four waves through LDS, and the workgroup's six doubles (3 channels
//                         x {cs, l*cs}) go to the caller's scratch.
//   msssim_pool_kernel    scale j -> j+1: 2x2 mean, stride 2, an odd last row / column paired with
//                         itself, on the float planes (scale 0 reads the uint8 arenas).
//   msssim_final_kernel   one wave per (image, scale) sums the tile partials in a fixed order.
//
// No floating-point atomics anywhere: the tiling of an image depends on its size only, every
// partial has its own slot and the final order is fixed, so the 30 doubles of an image are
// bit-identical from call to call and independent of the list around it and of its offset.
// E[xy] and E[xx] go through the same operations (contraction is off, every fma is written
// out), so identical inputs give cs = l = 1 exactly and sums equal to the position counts.
//
// The per-image table (at most kRagged images, 2.6 KB) is passed BY VALUE as in
// tic_image_batch.cpp: nothing is uploaded, the caller's host arrays are free on return and no
// call synchronises.  The pyramid planes and the partials live in the CALLER's scratch
// (tic_msssim_scratch_bytes): the handle struct belongs to tic_runtime.cpp, which stays as the
// shipped tuning states were stamped, so nothing here has a device-side lifetime.
//
// This file closes the one translation unit of the host runtime: it includes
// tic_image_batch.cpp (which includes tic_runtime.cpp) for the handle's stream and num_cus.
#include "tic_image_batch.cpp"

#pragma clang fp contract(off)

namespace tic {

constexpr int kMsScales = 5;
constexpr int kMsMinSide = 161;      // 161 -> 81 -> 41 -> 21 -> 11: one window at the last scale
constexpr int kMsMaxSide = 1 << 24;  // 3 * w stays far inside an int
constexpr int kMsTH = 16, kMsTW = 64;                   // output rows x interleaved elements per tile
constexpr int kMsVR = kMsTH / 4;                          // consecutive output rows per wave (4 waves)
constexpr int kMsRows = kMsTH + 10, kMsCols = kMsTW + 30;  // staged rows x elements (halo: 10 px = 30 elements)

struct MsTable {
  long long off[kRagged];       // first byte of image i in both uint8 arenas
  long long plane[kRagged];     // first float of image i's pyramid planes (scales 1..4, a then b per scale)
  long long part[kRagged];      // first double of image i's tile partials (scales 0..4, 6 per tile)
  long long base[kRagged + 1];  // items (tiles or pooled elements) of this launch before image i
  int H[kRagged], W[kRagged];
  int n;
};

// Size of scale j: ceil halving (an odd last row / column is paired with itself).
__host__ __device__ __forceinline__ int ms_dim(int n, int j) {
  for (int s = 0; s < j; ++s) n = (n + 1) >> 1;
  return n;
}
__host__ __device__ __forceinline__ long long ms_tiles(int h, int w) {
  return (long long)((h - 10 + kMsTH - 1) / kMsTH) * ((3 * (w - 10) + kMsTW - 1) / kMsTW);
}
// Floats before plane `which` (0 a, 1 b) of scale j >= 1 inside an image's plane block.
__host__ __device__ __forceinline__ long long ms_plane_off(int H, int W, int j, int which) {
  long long o = 0;
  for (int s = 1; s < j; ++s) o += 2LL * ms_dim(H, s) * ms_dim(W, s) * 3;
  return o + (long long)which * ms_dim(H, j) * ms_dim(W, j) * 3;
}
// Tiles before scale j inside an image's partial block.
__host__ __device__ __forceinline__ long long ms_tiles_before(int H, int W, int j) {
  long long o = 0;
  for (int s = 0; s < j; ++s) o += ms_tiles(ms_dim(H, s), ms_dim(W, s));
  return o;
}

// g[k] ~ exp(-(k-5)^2 / (2 * 1.5^2)), normalised in float64, rounded to float32
#define TIC_MS_G                                                                                        \
  {0.001028380123898387f, 0.0075987582094967365f, 0.036000773310661316f, 0.10936068743467331f,         \
   0.21300554275512695f,  0.26601171493530273f,   0.21300554275512695f,  0.10936068743467331f,         \
   0.036000773310661316f, 0.0075987582094967365f, 0.001028380123898387f}

template <bool U8>
__global__ void __launch_bounds__(256) msssim_scale_kernel(const MsTable t, const uint8_t* __restrict__ a8,
                                                           const uint8_t* __restrict__ b8,
                                                           const float* __restrict__ planes, int j,
                                                           double* __restrict__ part) {
  __shared__ float sA[kMsRows][kMsCols];
  __shared__ float sB[kMsRows][kMsCols];
  __shared__ float sM[5][kMsRows][kMsTW];
  __shared__ double sR[4][6];
  constexpr float g[11] = TIC_MS_G;

  const int i = ragged_find(t.base, t.n, (long long)blockIdx.x);
  const int tile = (int)((long long)blockIdx.x - t.base[i]);
  const int H = t.H[i], W = t.W[i];
  const int h = ms_dim(H, j), w = ms_dim(W, j);
  const int row_e = 3 * w, oh = h - 10, ow = 3 * (w - 10);
  const int tnx = (ow + kMsTW - 1) / kMsTW;
  const int y0 = (tile / tnx) * kMsTH, x0 = (tile % tnx) * kMsTW;
  const int tid = threadIdx.x;

  const uint8_t* pa8 = a8 + t.off[i];
  const uint8_t* pb8 = b8 + t.off[i];
  const float* pa = planes + t.plane[i] + ms_plane_off(H, W, j, 0);
  const float* pb = planes + t.plane[i] + ms_plane_off(H, W, j, 1);

  // stage both tiles with their halo, centred on 127.5; outside the image: 0 (feeds no valid output)
  for (int idx = tid; idx < kMsRows * kMsCols; idx += 256) {
    const int r = idx / kMsCols, c = idx - r * kMsCols;
    const int y = y0 + r, x = x0 + c;
    float va = 0.f, vb = 0.f;
    if (y < h && x < row_e) {
      const size_t o = (size_t)y * row_e + x;
      if (U8) {
        va = (float)pa8[o] - 127.5f;
        vb = (float)pb8[o] - 127.5f;
      } else {
        va = pa[o];
        vb = pb[o];
      }
    }
    sA[r][c] = va;
    sB[r][c] = vb;
  }
  __syncthreads();

  // horizontal pass: the five moments of every staged row (tap stride 3 elements = 1 pixel)
  for (int idx = tid; idx < kMsRows * kMsTW; idx += 256) {
    const int r = idx / kMsTW, c = idx - r * kMsTW;
    float ma = 0.f, mb = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float a = sA[r][c + 3 * k], b = sB[r][c + 3 * k];
      ma = fmaf(g[k], a, ma);
      mb = fmaf(g[k], b, mb);
      aa = fmaf(g[k], a * a, aa);
      bb = fmaf(g[k], b * b, bb);
      ab = fmaf(g[k], a * b, ab);
    }
    sM[0][r][c] = ma;
    sM[1][r][c] = mb;
    sM[2][r][c] = aa;
    sM[3][r][c] = bb;
    sM[4][r][c] = ab;
  }
  __syncthreads();

  // vertical pass and the per-position values; a thread keeps its column, hence its channel
  const int c = tid & 63;
  const int ch = (x0 + c) % 3;
  double dcs = 0.0, dl = 0.0;
  if (x0 + c < ow) {
    // a wave takes kMsVR consecutive output rows: their 11-row windows overlap, so the 14 staged
    // rows are read once and each feeds up to four accumulators (taps in ascending order)
    const int rb = (tid >> 6) * kMsVR;
    float acc[kMsVR][5];
#pragma unroll
    for (int q = 0; q < kMsVR; ++q) {
#pragma unroll
      for (int m = 0; m < 5; ++m) acc[q][m] = 0.f;
    }
#pragma unroll
    for (int rr = 0; rr < kMsVR + 10; ++rr) {
      float mv[5];
#pragma unroll
      for (int m = 0; m < 5; ++m) mv[m] = sM[m][rb + rr][c];
#pragma unroll
      for (int q = 0; q < kMsVR; ++q) {
        const int k = rr - q;
        if (k >= 0 && k < 11) {
#pragma unroll
          for (int m = 0; m < 5; ++m) acc[q][m] = fmaf(g[k], mv[m], acc[q][m]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < kMsVR; ++q) {
      if (y0 + rb + q >= oh) break;
      const float ma = acc[q][0], mb = acc[q][1], aa = acc[q][2], bb = acc[q][3], ab = acc[q][4];
      const float C1 = 6.5025f, C2 = 58.5225f;
      const float sxx = aa - ma * ma, syy = bb - mb * mb, sxy = ab - ma * mb;
      const float cs = (2.f * sxy + C2) / (sxx + syy + C2);
      const float ux = ma + 127.5f, uy = mb + 127.5f;
      const float l = (2.f * (ux * uy) + C1) / (ux * ux + uy * uy + C1);
      dcs += (double)cs;
      dl += (double)(l * cs);
    }
  }

  // workgroup sums per channel in a fixed order: lanes by shuffle, then the four waves
  double v[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) v[k] = (k >> 1) == ch ? ((k & 1) ? dl : dcs) : 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) sR[tid >> 6][k] = v[k];
  }
  __syncthreads();
  if (tid < 6)
    part[t.part[i] + 6 * (ms_tiles_before(H, W, j) + tile) + tid] = ((sR[0][tid] + sR[1][tid]) + sR[2][tid]) + sR[3][tid];
}

// One thread per element of scale j + 1 (both images); reads scale j.
template <bool U8>
__global__ void __launch_bounds__(256) msssim_pool_kernel(const MsTable t, const uint8_t* __restrict__ a8,
                                                          const uint8_t* __restrict__ b8, float* __restrict__ planes,
                                                          int j) {
  const size_t total = (size_t)t.base[t.n];
  for (size_t e = blockIdx.x * (size_t)256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int i = ragged_find(t.base, t.n, (long long)e);
    const size_t le = e - (size_t)t.base[i];
    const int H = t.H[i], W = t.W[i];
    const int h = ms_dim(H, j), w = ms_dim(W, j);
    const int w2 = (w + 1) >> 1;
    const size_t pix = le / 3;
    const int ch = (int)(le - pix * 3);
    const int y = (int)(pix / w2), x = (int)(pix - (size_t)y * w2);
    const int ya = 2 * y, yb = min(2 * y + 1, h - 1), xa = 2 * x, xb = min(2 * x + 1, w - 1);
    const size_t o00 = ((size_t)ya * w + xa) * 3 + ch, o01 = ((size_t)ya * w + xb) * 3 + ch;
    const size_t o10 = ((size_t)yb * w + xa) * 3 + ch, o11 = ((size_t)yb * w + xb) * 3 + ch;
    float* base = planes + t.plane[i];
    float* da = base + ms_plane_off(H, W, j + 1, 0);
    float* db = base + ms_plane_off(H, W, j + 1, 1);
    float ra, rb;
    if (U8) {
      const uint8_t* pa = a8 + t.off[i];
      const uint8_t* pb = b8 + t.off[i];
      ra = ((((float)pa[o00] - 127.5f) + ((float)pa[o01] - 127.5f)) + ((float)pa[o10] - 127.5f)) + ((float)pa[o11] - 127.5f);
      rb = ((((float)pb[o00] - 127.5f) + ((float)pb[o01] - 127.5f)) + ((float)pb[o10] - 127.5f)) + ((float)pb[o11] - 127.5f);
    } else {
      const float* pa = base + ms_plane_off(H, W, j, 0);
      const float* pb = base + ms_plane_off(H, W, j, 1);
      ra = ((pa[o00] + pa[o01]) + pa[o10]) + pa[o11];
      rb = ((pb[o00] + pb[o01]) + pb[o10]) + pb[o11];
    }
    da[le] = 0.25f * ra;
    db[le] = 0.25f * rb;
  }
}

// blockIdx.x: scale, blockIdx.y: image of this launch; one wave.  Lane l sums tiles l, l + 64, ...
// in order, then the lanes are folded by shuffle: the order depends on the tile count only.
__global__ void __launch_bounds__(64) msssim_final_kernel(const MsTable t, const double* __restrict__ part,
                                                          double* __restrict__ out) {
  const int j = blockIdx.x, i = blockIdx.y;
  const int H = t.H[i], W = t.W[i];
  const long long n = ms_tiles(ms_dim(H, j), ms_dim(W, j));
  const double* p = part + t.part[i] + 6 * ms_tiles_before(H, W, j);
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long long k = threadIdx.x; k < n; k += 64) {
#pragma unroll
    for (int q = 0; q < 6; ++q) v[q] += p[6 * k + q];
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_down(v[q], off, 64);
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < 6; ++q) out[((size_t)i * kMsScales + j) * 6 + q] = v[q];
  }
}

}  // namespace tic

namespace {

// Argument checks that need no device.
int ms_check_sizes(const int32_t* heights, const int32_t* widths, int n_images) {
  if (n_images < 0) return fail(TIC_EINVAL, "n_images %d is negative", n_images);
  if (n_images > 0 && (!heights || !widths)) return fail(TIC_EINVAL, "null per-image array");
  for (int i = 0; i < n_images; ++i) {
    if (heights[i] < tic::kMsMinSide || widths[i] < tic::kMsMinSide)
      return fail(TIC_EINVAL, "image %d: size %d x %d, MS-SSIM needs both sides >= %d (five scales of an 11x11 window)",
                  i, heights[i], widths[i], tic::kMsMinSide);
    if (heights[i] > tic::kMsMaxSide || widths[i] > tic::kMsMaxSide)
      return fail(TIC_EINVAL, "image %d: size %d x %d exceeds %d", i, heights[i], widths[i], tic::kMsMaxSide);
  }
  return TIC_OK;
}

// Doubles of partials and floats of planes one image needs.
void ms_image_need(int H, int W, long long* part_doubles, long long* plane_floats) {
  *part_doubles = 6 * tic::ms_tiles_before(H, W, tic::kMsScales);
  *plane_floats = tic::ms_plane_off(H, W, tic::kMsScales, 0);
}

size_t ms_scratch(const int32_t* heights, const int32_t* widths, int n_images) {
  size_t bytes = 0;
  for (int i = 0; i < n_images; ++i) {
    long long pd, pf;
    ms_image_need(heights[i], widths[i], &pd, &pf);
    bytes += (size_t)pd * sizeof(double) + (size_t)pf * sizeof(float);
  }
  return bytes;
}

}  // namespace

extern "C" {

int tic_msssim_scratch_bytes(const int32_t* heights, const int32_t* widths, int n_images, size_t* bytes) {
  if (!bytes) return fail(TIC_EINVAL, "null bytes");
  *bytes = 0;
  if (!heights || !widths) return fail(TIC_EINVAL, "null per-image array");
  int rc = ms_check_sizes(heights, widths, n_images);
  if (rc) return rc;
  *bytes = ms_scratch(heights, widths, n_images);
  return TIC_OK;
}

int tic_msssim_images_device(tic_handle* h, const uint8_t* d_a, const uint8_t* d_b, const int64_t* offsets,
                             const int32_t* heights, const int32_t* widths, int n_images, void* d_scratch,
                             size_t scratch_bytes, double* d_out) {
  if (!h) return fail(TIC_EINVAL, "null handle");
  if (n_images < 0) return fail(TIC_EINVAL, "n_images %d is negative", n_images);
  if (n_images == 0) return TIC_OK;
  if (!d_a || !d_b || !d_scratch || !d_out) return fail(TIC_EINVAL, "null device pointer");
  if (!offsets) return fail(TIC_EINVAL, "null per-image array");
  int rc = ms_check_sizes(heights, widths, n_images);
  if (rc) return rc;
  for (int i = 0; i < n_images; ++i)
    if (offsets[i] < 0) return fail(TIC_EINVAL, "image %d: negative offset %lld", i, (long long)offsets[i]);
  if (((uintptr_t)d_scratch & 7) != 0 || ((uintptr_t)d_out & 7) != 0)
    return fail(TIC_EINVAL, "d_scratch and d_out must be 8-byte aligned");
  const size_t need = ms_scratch(heights, widths, n_images);
  if (scratch_bytes < need)
    return fail(TIC_EINVAL, "scratch of %zu bytes is too small (tic_msssim_scratch_bytes: %zu)", scratch_bytes, need);

  // scratch: the partials (doubles) of all images, then the planes (floats) of all images
  long long part_total = 0;
  for (int i = 0; i < n_images; ++i) {
    long long pd, pf;
    ms_image_need(heights[i], widths[i], &pd, &pf);
    part_total += pd;
  }
  double* d_part = static_cast<double*>(d_scratch);
  float* d_planes = reinterpret_cast<float*>(d_part + part_total);

  // every launch's item count must fit the grid / an int tile index
  for (int s = 0; s < n_images; s += tic::kRagged) {
    long long tiles0 = 0;
    for (int i = s; i < std::min(n_images, s + tic::kRagged); ++i) tiles0 += tic::ms_tiles(heights[i], widths[i]);
    if (tiles0 > INT_MAX) return fail(TIC_EINVAL, "more than 2^31 - 1 tiles in one launch");
  }

  HIP_TRY(hipSetDevice(h->device));
  long long part_at = 0, plane_at = 0;
  for (int s = 0; s < n_images; s += tic::kRagged) {
    tic::MsTable t;
    memset(&t, 0, sizeof(t));
    t.n = std::min(tic::kRagged, n_images - s);
    for (int k = 0; k < t.n; ++k) {
      const int i = s + k;
      long long pd, pf;
      ms_image_need(heights[i], widths[i], &pd, &pf);
      t.off[k] = offsets[i];
      t.H[k] = heights[i];
      t.W[k] = widths[i];
      t.part[k] = part_at;
      t.plane[k] = plane_at;
      part_at += pd;
      plane_at += pf;
    }
    for (int j = 0; j < tic::kMsScales; ++j) {
      long long tiles = 0;
      for (int k = 0; k < t.n; ++k) {
        t.base[k] = tiles;
        tiles += tic::ms_tiles(tic::ms_dim(t.H[k], j), tic::ms_dim(t.W[k], j));
      }
      t.base[t.n] = tiles;
      touch(h);
      if (j == 0)
        hipLaunchKernelGGL(tic::msssim_scale_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, h->stream, t, d_a, d_b,
                           (const float*)d_planes, j, d_part);
      else
        hipLaunchKernelGGL(tic::msssim_scale_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, h->stream, t, d_a,
                           d_b, (const float*)d_planes, j, d_part);
      if ((rc = check_launch())) return rc;
      if (j + 1 == tic::kMsScales) break;
      long long elems = 0;
      for (int k = 0; k < t.n; ++k) {
        t.base[k] = elems;
        elems += (long long)tic::ms_dim(t.H[k], j + 1) * tic::ms_dim(t.W[k], j + 1) * 3;
      }
      t.base[t.n] = elems;
      const unsigned grid = tic::ragged_grid((size_t)elems, h->num_cus);
      if (j == 0)
        hipLaunchKernelGGL(tic::msssim_pool_kernel<true>, dim3(grid), dim3(256), 0, h->stream, t, d_a, d_b, d_planes,
                           j);
      else
        hipLaunchKernelGGL(tic::msssim_pool_kernel<false>, dim3(grid), dim3(256), 0, h->stream, t, d_a, d_b, d_planes,
                           j);
      if ((rc = check_launch())) return rc;
    }
    hipLaunchKernelGGL(tic::msssim_final_kernel, dim3(tic::kMsScales, t.n), dim3(64), 0, h->stream, t,
                       (const double*)d_part, d_out + (size_t)s * tic::kMsScales * 6);
    if ((rc = check_launch())) return rc;
  }
  return TIC_OK;
}

}  // extern "C"
