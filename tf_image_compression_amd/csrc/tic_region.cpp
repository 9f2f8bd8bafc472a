// tic_region.cpp — decoding a rectangle of an image: which patches it needs (tic_region_plan), the
// block-effect post-filter on a part of an image (tic_rmbe_regions_device) and the final crop
// (tic_crop_regions_device); include/tic.h has the contracts.
//
// Patches are independent and so are the segments of a container, so a crop of h x w pixels needs
// the patches it touches and, with the post-filter, those its windows reach.  The patches of that
// box, row-major, are the patch batch of an image of the box's size: the decoder, the stitch and
// the rounding run on them unchanged.  What is new is that the post-filter's windows must keep
// their places in the FULL image's grid while only a part of the image exists:
//
//   window_copy_region_kernel   window_copy_ragged_kernel with a per-region origin: the table
//                               carries, for each region, the local position of its first window
//                               of the pass and the windows per row that lie wholly inside it
//   crop_region_kernel          rows [y, y + h) x columns [x, x + w) of every uint8 HWC box into a
//                               dense [h, w, 3] block, one thread per output byte
//
// Same style as tic_image_batch.cpp: tables BY VALUE in the kernel arguments, host arrays free on
// return, nothing uploaded, no call synchronises; a list longer than kRagged runs as several
// launches.  This file closes the one translation unit of the host runtime (it includes
// tic_entropy.cpp, which includes tic_msssim.cpp, tic_image_batch.cpp and tic_runtime.cpp).
#include "tic_entropy.cpp"

namespace tic {

struct RegionTable {
  long long off[kRagged];   // first element of region i in the arena
  long long obase[kRagged + 1];  // crop: output bytes before region i
  long long ooff[kRagged];  // crop: first byte of region i's output
  int pbase[kRagged + 1];   // windows before region i
  int W[kRagged];           // the region's own width (its row pitch in pixels)
  int wn[kRagged];          // windows per row inside region i
  int r0[kRagged], c0[kRagged];  // local row / column of its first window; crop: of the crop
  int cw[kRagged];          // crop: width of the crop
  int n;
};

// Windows [sum hn_i*wn_i, S, S, 3] <-> regions of the arena at local (r0_i + j*S, c0_i + k*S).
// to_windows: gather (regions -> windows); else scatter (windows -> regions, in place).
__global__ void __launch_bounds__(256) window_copy_region_kernel(const RegionTable t, float* __restrict__ arena,
                                                                 int S, size_t total, float* __restrict__ win,
                                                                 int to_windows) {
  const size_t row = (size_t)S * 3, wsz = row * S;
  for (size_t e = blockIdx.x * (size_t)256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int gp = (int)(e / wsz);
    const int i = ragged_find(t.pbase, t.n, gp);
    const int p = gp - t.pbase[i];
    const int wn = t.wn[i];
    const size_t rem = e - (size_t)gp * wsz;
    const int y = (int)(rem / row);
    const int xc = (int)(rem - (size_t)y * row);
    const size_t o =
        (size_t)t.off[i] + ((size_t)(t.r0[i] + (p / wn) * S + y) * t.W[i] + t.c0[i] + (p % wn) * S) * 3 + xc;
    if (to_windows) win[e] = arena[o];
    else arena[o] = win[e];
  }
}

// One thread per output byte: out[ooff_i + (r * cw_i + c) * 3 + k] = box_i[r0_i + r][c0_i + c][k].
__global__ void __launch_bounds__(256) crop_region_kernel(const RegionTable t, const uint8_t* __restrict__ arena,
                                                          uint8_t* __restrict__ out) {
  const size_t total = (size_t)t.obase[t.n];
  for (size_t g = blockIdx.x * (size_t)256 + threadIdx.x; g < total; g += (size_t)gridDim.x * 256) {
    const int i = ragged_find(t.obase, t.n, (long long)g);
    const size_t e = g - (size_t)t.obase[i];
    const size_t rowb = (size_t)t.cw[i] * 3;
    const size_t r = e / rowb, cb = e - r * rowb;
    out[t.ooff[i] + (long long)e] = arena[(size_t)t.off[i] + ((size_t)(t.r0[i] + r) * t.W[i] + t.c0[i]) * 3 + cb];
  }
}

}  // namespace tic

namespace {

// [lo, hi) extended over every band [start + a*S, start + a*S + S), 0 <= a < count, it intersects.
void region_extend(long long* lo, long long* hi, long long start, long long S, long long count) {
  if (count <= 0 || *hi <= start) return;
  const long long a0 = *lo > start ? (*lo - start) / S : 0;
  const long long a1 = std::min(count - 1, (*hi - 1 - start) / S);
  if (a0 > a1) return;  // the range lies behind the last band
  *lo = std::min(*lo, start + a0 * S);
  *hi = std::max(*hi, start + a1 * S + S);
}

// The full-grid windows of one rmbe pass that lie wholly inside a region: first index and count
// along one axis.  start: the pass's offset on this axis; full, o, len: the full image's size, the
// region's origin and its size on this axis.
void region_windows(int start, int S, int full, int o, int len, int* first, int* count) {
  const int total = full >= start ? (full - start) / S : 0;
  int a0 = o > start ? (o - start + S - 1) / S : 0;
  int a1 = o + len >= start ? (o + len - start) / S : 0;  // exclusive
  a1 = std::min(a1, total);
  *first = a0;
  *count = std::max(0, a1 - a0);
}

}  // namespace

extern "C" {

int tic_region_plan(int H, int W, int P, int y, int x, int h, int w, int S, int* py0, int* py1, int* px0, int* px1) {
  if (!py0 || !py1 || !px0 || !px1) return fail(TIC_EINVAL, "null output");
  *py0 = *py1 = *px0 = *px1 = 0;
  if (H <= 0 || W <= 0) return fail(TIC_EINVAL, "image size %d x %d must be positive", H, W);
  if (P <= 0) return fail(TIC_EINVAL, "P %d must be positive", P);
  if (S < 0 || (S & 1)) return fail(TIC_EINVAL, "window side %d must be even and not negative", S);
  if (h <= 0 || w <= 0) return fail(TIC_EINVAL, "region %d x %d is empty", h, w);
  if (y < 0 || x < 0 || y > H - h || x > W - w)
    return fail(TIC_EINVAL, "region %d x %d at (%d, %d) is not inside the image of %d x %d", h, w, y, x, H, W);
  long long r0 = y, r1 = (long long)y + h, c0 = x, c1 = (long long)x + w;
  if (S > 0) {
    const int o = S / 2;
    region_extend(&r0, &r1, o, S, H >= o ? (H - o) / S : 0);  // pass 2: row offset o
    region_extend(&r0, &r1, 0, S, H / S);                     // pass 1: row offset 0
    region_extend(&c0, &c1, 0, S, W / S);                     // pass 2: column offset 0
    region_extend(&c0, &c1, o, S, W >= o ? (W - o) / S : 0);  // pass 1: column offset o
  }
  *py0 = (int)(r0 / P);
  *py1 = (int)std::min<long long>((r1 + P - 1) / P, ((long long)H + P - 1) / P);
  *px0 = (int)(c0 / P);
  *px1 = (int)std::min<long long>((c1 + P - 1) / P, ((long long)W + P - 1) / P);
  return TIC_OK;
}

int tic_rmbe_regions_device(tic_handle* h, float* d_arena, const int64_t* offsets, const int32_t* heights,
                            const int32_t* widths, const int32_t* y0s, const int32_t* x0s,
                            const int32_t* full_heights, const int32_t* full_widths, int n) {
  if (!h) return fail(TIC_EINVAL, "null handle");
  if (n < 0) return fail(TIC_EINVAL, "n %d is negative", n);
  if (n == 0) return TIC_OK;
  if (!d_arena) return fail(TIC_EINVAL, "null device pointer");
  if (!y0s || !x0s || !full_heights || !full_widths) return fail(TIC_EINVAL, "null per-region array");
  int rc = ragged_check(offsets, heights, widths, n);
  if (!rc) rc = ragged_disjoint(offsets, heights, widths, n);
  if (rc) return rc;
  for (int i = 0; i < n; ++i)
    if (y0s[i] < 0 || x0s[i] < 0 || full_heights[i] <= 0 || full_widths[i] <= 0 ||
        y0s[i] > full_heights[i] - heights[i] || x0s[i] > full_widths[i] - widths[i])
      return fail(TIC_EINVAL, "region %d: %d x %d at (%d, %d) is not inside the image of %d x %d", i, heights[i],
                  widths[i], y0s[i], x0s[i], full_heights[i], full_widths[i]);
  if (!h->rmbe()) return fail(TIC_EINVAL, "handle is not an rmbe handle");
  if ((rc = check_ready(h))) return rc;
  const int S = h->P, off = S / 2;
  const size_t wsz = (size_t)S * S * 3;
  for (int pass = 0; pass < 2; ++pass) {
    // the pass's window grid is the full image's (tic_rmbe_image_device); a region takes the
    // windows of it that lie wholly inside
    const int r0 = pass == 0 ? 0 : off, c0 = pass == 0 ? off : 0;
    struct Win {
      int a0, hn, b0, wn;
    };
    std::vector<Win> wins(n);
    long long total = 0;
    for (int i = 0; i < n; ++i) {
      Win& q = wins[i];
      region_windows(r0, S, full_heights[i], y0s[i], heights[i], &q.a0, &q.hn);
      region_windows(c0, S, full_widths[i], x0s[i], widths[i], &q.b0, &q.wn);
      if (q.hn == 0 || q.wn == 0) q.hn = q.wn = 0;
      total += (long long)q.hn * q.wn;
      if (total > INT_MAX) return fail(TIC_EINVAL, "more than 2^31 - 1 windows");
    }
    if (total == 0) continue;
    const size_t bytes = (size_t)total * wsz * sizeof(float);
    rc = ensure(&h->win_in, &h->win_in_bytes, bytes);
    if (!rc) rc = ensure(&h->win_out, &h->win_out_bytes, bytes);
    if (rc) return rc;
    auto copy = [&](float* win, int to_windows) {
      long long before = 0;
      for (int s = 0; s < n; s += tic::kRagged) {
        tic::RegionTable t;
        memset(&t, 0, sizeof(t));
        t.n = std::min(tic::kRagged, n - s);
        long long items = 0;
        for (int k = 0; k < t.n; ++k) {
          const int i = s + k;
          t.off[k] = offsets[i];
          t.W[k] = widths[i];
          t.wn[k] = std::max(1, wins[i].wn);
          t.r0[k] = r0 + wins[i].a0 * S - y0s[i];
          t.c0[k] = c0 + wins[i].b0 * S - x0s[i];
          t.pbase[k] = (int)items;
          items += (long long)wins[i].hn * wins[i].wn;
        }
        t.pbase[t.n] = (int)items;
        if (items > 0) {
          const size_t elems = (size_t)items * wsz;
          touch(h);
          hipLaunchKernelGGL(tic::window_copy_region_kernel, dim3(tic::ragged_grid(elems, h->num_cus)), dim3(256), 0,
                             h->stream, t, d_arena, S, elems, win + (size_t)before * wsz, to_windows);
          const int lrc = check_launch();
          if (lrc) return lrc;
        }
        before += items;
      }
      return (int)TIC_OK;
    };
    if ((rc = copy((float*)h->win_in, 1))) return rc;
    if ((rc = rmbe_dev(h, (const float*)h->win_in, (int)total, (float*)h->win_out, Prof{nullptr}))) return rc;
    if ((rc = copy((float*)h->win_out, 0))) return rc;
  }
  return TIC_OK;
}

int tic_crop_regions_device(tic_handle* h, const uint8_t* d_boxes, const int64_t* offsets, const int32_t* heights,
                            const int32_t* widths, const int32_t* ys, const int32_t* xs, const int32_t* hs,
                            const int32_t* ws, const int64_t* out_offsets, int n, uint8_t* d_out) {
  if (!h) return fail(TIC_EINVAL, "null handle");
  if (n < 0) return fail(TIC_EINVAL, "n %d is negative", n);
  if (n == 0) return TIC_OK;
  if (!d_boxes || !d_out) return fail(TIC_EINVAL, "null device pointer");
  if (!ys || !xs || !hs || !ws || !out_offsets) return fail(TIC_EINVAL, "null per-region array");
  int rc = ragged_check(offsets, heights, widths, n);
  if (rc) return rc;
  for (int i = 0; i < n; ++i) {
    if (hs[i] <= 0 || ws[i] <= 0 || ys[i] < 0 || xs[i] < 0 || ys[i] > heights[i] - hs[i] || xs[i] > widths[i] - ws[i])
      return fail(TIC_EINVAL, "crop %d: %d x %d at (%d, %d) is not inside the box of %d x %d", i, hs[i], ws[i], ys[i],
                  xs[i], heights[i], widths[i]);
    if (out_offsets[i] < 0) return fail(TIC_EINVAL, "crop %d: negative output offset", i);
  }
  if ((rc = ragged_disjoint(out_offsets, hs, ws, n))) return rc;
  HIP_TRY(hipSetDevice(h->device));
  for (int s = 0; s < n; s += tic::kRagged) {
    tic::RegionTable t;
    memset(&t, 0, sizeof(t));
    t.n = std::min(tic::kRagged, n - s);
    long long bytes = 0;
    for (int k = 0; k < t.n; ++k) {
      const int i = s + k;
      t.off[k] = offsets[i];
      t.W[k] = widths[i];
      t.r0[k] = ys[i];
      t.c0[k] = xs[i];
      t.cw[k] = ws[i];
      t.ooff[k] = out_offsets[i];
      t.obase[k] = bytes;
      bytes += (long long)hs[i] * ws[i] * 3;
    }
    t.obase[t.n] = bytes;
    touch(h);
    hipLaunchKernelGGL(tic::crop_region_kernel, dim3(tic::ragged_grid((size_t)bytes, h->num_cus)), dim3(256), 0,
                       h->stream, t, d_boxes, d_out);
    if ((rc = check_launch())) return rc;
  }
  return TIC_OK;
}

}  // extern "C"
