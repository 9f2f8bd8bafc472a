// tic_entropy.cpp — the segmented range-coder stream (include/tic.h, "TICS" versions 1 to 3) coded on
// the device, and its C-ABI entries.
//
// The single-stream coder of range_coder.cpp is one latency chain per image.  A segmented stream
// cuts the symbols into segments of L that are independent range-coder streams, so the chain is
// L symbols long and there are n / L of them:
//
//   ent_encode_kernel       ONE SEGMENT PER LANE, 64-lane workgroups (a latency chain, not a
//                           bandwidth kernel: waves spread over the CUs).  The coder state (low,
//                           range, cache, pending) stays in registers; carries are resolved with
//                           the host's cache + pending-0xFF scheme, so no stored byte is revisited.
//                           A lane reads its own symbols with 16-byte loads once its address is
//                           aligned and writes its payload, four bytes per store, into its own
//                           slot of the scratch (stride 3L + 4, the worst case) and its length
//                           beside it.
//   ent_seg_scan_kernel     one workgroup per stream: exclusive scan of its segment lengths, the
//                           container size into d_sizes (UINT64_MAX when a lane met a symbol
//                           outside the table)
//   ent_stream_scan_kernel  one workgroup: exclusive scan over the streams
//   ent_gather_kernel       one workgroup per segment: consecutive threads copy consecutive
//                           payload bytes to their final place; the first segment's workgroup also
//                           writes the header, every workgroup its u16 length
//
// and the decoder: ent_dec_header_kernel (checks each header against the caller's count and
// size), ent_stream_scan_kernel over the segment counts, ent_dec_scan_kernel (segment offsets;
// zero-fills a stream it cannot decode) and ent_decode_kernel (one segment per lane, grid-stride).
//
// Arithmetic is the host's, exactly: range needs 33 bits (it starts at 2^32) and is held in 64;
// range / total is a shift when the total is a power of two and a true division otherwise; the
// decoder's code / r is a true 32-bit division (r = 2^32 only when the total is 1, where the
// quotient is 0).  The decoder finds the symbol of a value through a byte table in LDS built by
// each workgroup from the cumulative table (totals up to 65536), else by the host's binary search.
//
// The model (at most 257 cumulative counts) and the per-stream tables travel BY VALUE in kernel
// arguments, as in tic_image_batch.cpp: nothing is uploaded, host arrays are free on return and
// no call synchronises.  The per-stream records a later kernel needs are written to the caller's
// scratch by a kernel that received them by value.  tic_entropy_set_table therefore only keeps
// the validated table on the host, keyed by the handle; the handle struct belongs to
// tic_runtime.cpp, which stays as the shipped tuning states were stamped, so tic_destroy is
// wrapped below to drop that entry with the handle.
//
// Version 2 of the container (a periodic context model: K tables, symbol k of a stream under table
// k mod K; 28-byte header with K and the tables' CRC-32C) runs through the same launches.  The
// scan, gather and header kernels are templates over the header size; the coder kernels have
// context variants, ent_encode_ctx_kernel / ent_decode_ctx_kernel, below the version-1 ones, which
// stay as they were.  K tables do not fit kernel arguments: tic_entropy_set_tables uploads them to
// a device buffer kept in the same per-handle entry, which the tic_destroy wrapper frees.
// ent_histogram_ctx_kernel counts symbols per context for estimating such tables.
//
// Version 3 (K0 periodic contexts x the classes of a symbol's causal neighbours; 36-byte header
// with K0, the CRC, the code geometry and `neighbours`) is a third instance of the templates and
// a third pair of coder kernels, ent_encode_nbr_kernel / ent_decode_nbr_kernel, with
// ent_histogram_nbr_kernel for its tables; they follow the version-2 kernels below.
//
// Symbol ranges (tic_entropy_decode_ranges*_device): the decoder's kernels are templates over RNG.
// RNG = 0 decodes whole containers, the code the entries above have always launched; RNG = 1 takes
// one range [first, first + count) per record, the work items being the segments of all ranges
// (struct EntRng below).  There is no second copy of the decode arithmetic for them.
//
// This file is part of the one translation unit of the host runtime: it includes tic_msssim.cpp,
// and tic_region.cpp includes it.
#define tic_destroy tic_destroy_runtime_
#include "tic_msssim.cpp"
#undef tic_destroy

#include <mutex>

namespace tic {

constexpr int kEntStreams = 64;  // streams per by-value table
constexpr uint32_t kEntMaxL = 16384;
constexpr uint32_t kEntBad = 0xFFFFFFFFu;
constexpr uint32_t kEntLutMax = 65536;

struct EntModel {
  uint32_t cum[257];
  int nsym;
  int shift;  // log2(total) when the total is a power of two, else -1
};

struct EntChunk {
  long long in_off[kEntStreams], in_size[kEntStreams], count[kEntStreams], out_off[kEntStreams];
  long long seg_base[kEntStreams + 1];
  int n, first, last;  // last: this chunk ends the list (seg_base[n] is the total)
};

struct EntRec {
  long long in_off, in_size, count, out_off;
  uint32_t L, valid;
};

// A symbol range [first, first + count) of a container (tic_entropy_decode_ranges*_device).  The
// decoder's kernels are templates over RNG: 0 decodes whole containers and is the code the
// entries without ranges have always launched (the trailing range arguments are never read);
// 1 takes one range per record, its work items being the segments first / L ..
// (first + count - 1) / L of the range's container.
struct EntRng {
  long long first, count;
};
// The ranges of one chunk of records, by value beside EntChunk; nothing for RNG = 0.
template <int RNG>
struct EntRngChunk {
  long long first[kEntStreams], count[kEntStreams];
};
template <>
struct EntRngChunk<0> {};

__host__ __device__ __forceinline__ uint32_t ent_stride(uint32_t L) { return 3 * L + 4; }

// Last i with base[i] <= v, base in device memory (ragged_find's contract).
__device__ __forceinline__ int ent_find(const unsigned long long* base, int n, unsigned long long v) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (base[mid] <= v) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Inclusive scan of one value per thread over a 256-thread workgroup (s: 256 entries).
__device__ __forceinline__ unsigned long long ent_block_scan(unsigned long long v, unsigned long long* s) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const unsigned long long o = t >= d ? s[t - d] : 0;
    __syncthreads();
    s[t] += o;
    __syncthreads();
  }
  const unsigned long long r = s[t];
  __syncthreads();
  return r;
}

// The by-value records of one chunk of streams into the scratch.
__global__ void __launch_bounds__(64) ent_put_kernel(const EntChunk t, uint32_t L, EntRec* __restrict__ rec,
                                                     unsigned long long* __restrict__ seg_base) {
  const int k = threadIdx.x;
  if (k < t.n) {
    EntRec r;
    r.in_off = t.in_off[k];
    r.in_size = t.in_size[k];
    r.count = t.count[k];
    r.out_off = t.out_off[k];
    r.L = L;
    r.valid = 1;
    rec[t.first + k] = r;
    seg_base[t.first + k] = (unsigned long long)t.seg_base[k];
  }
  if (k == 0 && t.last) seg_base[t.first + t.n] = (unsigned long long)t.seg_base[t.n];
}

// put / emit_top / the flush below have a second copy in ent_encode_ctx_kernel (this kernel stays
// as it was measured): a fix to the carry or flush logic goes into both.
__global__ void __launch_bounds__(64) ent_encode_kernel(const EntModel m, const uint8_t* __restrict__ sym,
                                                        const EntRec* __restrict__ rec,
                                                        const unsigned long long* __restrict__ seg_base, int n_streams,
                                                        uint32_t L, uint8_t* __restrict__ slots,
                                                        uint32_t* __restrict__ seg_len) {
  __shared__ uint32_t s_cum[257];
  for (int k = threadIdx.x; k <= m.nsym; k += 64) s_cum[k] = m.cum[k];
  __syncthreads();
  const unsigned long long T = seg_base[n_streams];
  const unsigned long long g = (unsigned long long)blockIdx.x * 64 + threadIdx.x;
  if (g >= T) return;
  const int i = ent_find(seg_base, n_streams, g);
  const unsigned long long j = g - seg_base[i];
  const long long left = rec[i].count - (long long)(j * L);
  const uint32_t cnt = left < (long long)L ? (uint32_t)left : L;
  const uint8_t* src = sym + rec[i].in_off + (long long)(j * L);
  uint32_t* out = reinterpret_cast<uint32_t*>(slots + (size_t)g * ent_stride(L));

  const uint32_t nsym = (uint32_t)m.nsym, total = m.cum[m.nsym];
  const int shift = m.shift;
  unsigned long long low = 0, range = 1ull << 32;
  int cache = -1;
  uint32_t pending = 0, nout = 0, acc = 0;
  bool bad = false;

  auto put = [&](uint32_t b) {
    acc |= (b & 0xFFu) << (8 * (nout & 3));
    ++nout;
    if ((nout & 3) == 0) {
      out[(nout >> 2) - 1] = acc;
      acc = 0;
    }
  };
  auto emit_top = [&]() {
    if (low < 0xFF000000ull || low >= (1ull << 32)) {
      const uint32_t carry = low >= (1ull << 32) ? 1u : 0u;
      if (cache >= 0) put((uint32_t)cache + carry);
      for (; pending; --pending) put(0xFFu + carry);
      cache = (int)((low >> 24) & 0xFF);
    } else {
      ++pending;
    }
    low = (low << 8) & 0xFFFFFFFFull;
  };
  auto step = [&](uint32_t s) {
    if (s >= nsym) {
      bad = true;
      return;
    }
    const uint32_t start = s_cum[s], next = s_cum[s + 1];
    unsigned long long r;
    if (shift >= 0) r = range >> shift;
    else if (range >> 32) r = range / total;
    else r = (uint32_t)range / total;
    const unsigned long long sr = (unsigned long long)start * r;
    low += sr;
    range = next == total ? range - sr : (unsigned long long)(next - start) * r;
    while (range < (1ull << 24)) {
      range <<= 8;
      emit_top();
    }
  };

  uint32_t k = 0;
  for (; k < cnt && ((uintptr_t)(src + k) & 15) != 0; ++k) step(src[k]);
  for (; k + 16 <= cnt; k += 16) {
    const uint4 v = *reinterpret_cast<const uint4*>(src + k);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t x = w[q];
#pragma unroll 1
      for (int b = 0; b < 4; ++b) {
        step(x & 0xFFu);
        x >>= 8;
      }
    }
  }
  for (; k < cnt; ++k) step(src[k]);

  // the minimal flush (range_coder.cpp EncCore::finish)
  int nb = 0;
  unsigned long long v = low;
  for (; nb <= 4; ++nb) {
    if (nb == 4) {
      v = low;
    } else {
      const unsigned long long unit = 1ull << (32 - 8 * nb);
      v = (low + unit - 1) & ~(unit - 1);
    }
    if (v < low + range) break;
  }
  low = v;
  for (int q = 0; q < nb; ++q) emit_top();
  if (nb > 0) {
    if (cache >= 0) put((uint32_t)cache);
    for (; pending; --pending) put(0xFFu);
  } else if (cache >= 0) {
    const uint32_t carry = v >= (1ull << 32) ? 1u : 0u;
    put((uint32_t)cache + carry);
    for (; pending; --pending) put(0xFFu + carry);
  }
  if (nout & 3) out[nout >> 2] = acc;  // the slot is a multiple of 4 bytes
  seg_len[g] = bad ? kEntBad : nout;
}

// Workgroup i: exclusive scan of stream i's segment lengths; its container size.  HDR: the
// header's bytes, 20 (version 1), 28 (version 2) or 36 (version 3), here and in the kernels below.
template <int HDR>
__global__ void __launch_bounds__(256) ent_seg_scan_kernel(const EntRec* __restrict__ rec,
                                                           const unsigned long long* __restrict__ seg_base,
                                                           const uint32_t* __restrict__ seg_len,
                                                           unsigned long long* __restrict__ seg_off,
                                                           unsigned long long* __restrict__ sizes) {
  __shared__ unsigned long long s[256];
  __shared__ int s_bad;
  const int i = blockIdx.x, t = threadIdx.x;
  const unsigned long long b = seg_base[i], S = seg_base[i + 1] - b;
  if (t == 0) s_bad = 0;
  __syncthreads();
  unsigned long long carry = 0;
  bool bad = false;
  for (unsigned long long j0 = 0; j0 < S; j0 += 256) {
    const unsigned long long j = j0 + t;
    uint32_t len = j < S ? seg_len[b + j] : 0;
    if (len == kEntBad) {
      bad = true;
      len = 0;
    }
    const unsigned long long inc = ent_block_scan(len, s);
    if (j < S) seg_off[b + j] = carry + inc - len;
    carry += s[255];
    __syncthreads();
  }
  if (bad) s_bad = 1;  // every writer stores the same value
  __syncthreads();
  if (t == 0) sizes[i] = s_bad ? ~0ull : (unsigned long long)HDR + 2ull * S + carry;
}

// One workgroup: out[i] = sum of in[k], k < i (UINT64_MAX counts as 0); out has n + 1 entries.
__global__ void __launch_bounds__(256) ent_stream_scan_kernel(const unsigned long long* __restrict__ in, int n,
                                                              unsigned long long* __restrict__ out) {
  __shared__ unsigned long long s[256];
  const int t = threadIdx.x;
  unsigned long long carry = 0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + t;
    unsigned long long v = i < n ? in[i] : 0;
    if (v == ~0ull) v = 0;
    const unsigned long long inc = ent_block_scan(v, s);
    if (i < n) out[i] = carry + inc - v;
    carry += s[255];
    __syncthreads();
  }
  if (t == 0) out[n] = carry;
}

// Workgroup g: segment g's payload, its length and (first segment) the header to their places.
// K, crc: the version-2 header's two words (unused by version 1); g0, g1: version 3's two more
// (eh | ew << 16, C | neighbours << 16), K then being K0.
template <int HDR>
__global__ void __launch_bounds__(256) ent_gather_kernel(const EntRec* __restrict__ rec,
                                                         const unsigned long long* __restrict__ seg_base,
                                                         int n_streams, uint32_t L, const uint8_t* __restrict__ slots,
                                                         const uint32_t* __restrict__ seg_len,
                                                         const unsigned long long* __restrict__ seg_off,
                                                         const unsigned long long* __restrict__ sizes,
                                                         const unsigned long long* __restrict__ out_off,
                                                         uint32_t K, uint32_t crc, uint32_t g0, uint32_t g1,
                                                         uint8_t* __restrict__ out) {
  const unsigned long long g = blockIdx.x;
  const int i = ent_find(seg_base, n_streams, g);
  if (sizes[i] == ~0ull) return;
  const unsigned long long j = g - seg_base[i], S = seg_base[i + 1] - seg_base[i];
  uint8_t* base = out + out_off[i];
  const int t = threadIdx.x;
  const uint32_t len = seg_len[g];
  if (j == 0 && t < HDR) {
    const unsigned long long n = (unsigned long long)rec[i].count;
    uint32_t b;
    if (t < 4) b = (0x53434954u >> (8 * t)) & 0xFFu;  // "TICS"
    else if (t < 8) b = t == 4 ? (HDR == 36 ? 3u : HDR == 28 ? 2u : 1u) : 0u;
    else if (t < 12) b = (L >> (8 * (t - 8))) & 0xFFu;
    else if (t < 20) b = (uint32_t)(n >> (8 * (t - 12))) & 0xFFu;
    else if (t < 24) b = (K >> (8 * (t - 20))) & 0xFFu;
    else if (t < 28) b = (crc >> (8 * (t - 24))) & 0xFFu;
    else if (t < 32) b = (g0 >> (8 * (t - 28))) & 0xFFu;
    else b = (g1 >> (8 * (t - 32))) & 0xFFu;
    base[t] = (uint8_t)b;
  }
  if (t < 2) base[HDR + 2 * j + t] = (uint8_t)(len >> (8 * t));
  const uint8_t* src = slots + (size_t)g * ent_stride(L);
  uint8_t* dst = base + HDR + 2 * S + seg_off[g];
  for (uint32_t k = t; k < len; k += 256) dst[k] = src[k];
}

// Lane k: the header of container first + k against the caller's count and size and, version 2,
// against the K and the CRC of the tables set and, version 3, the geometry words g0, g1 as well.
// RNG: record k is a range of its container; seg_cnt receives the segments the range touches, and a
// range that is empty or not inside the header's n makes the record invalid.
template <int HDR, int RNG>
__global__ void __launch_bounds__(64) ent_dec_header_kernel(const EntChunk t, const uint8_t* __restrict__ blob,
                                                            uint32_t K, uint32_t crc, uint32_t g0, uint32_t g1,
                                                            EntRec* __restrict__ rec,
                                                            unsigned long long* __restrict__ seg_cnt,
                                                            const EntRngChunk<RNG> rg, EntRng* __restrict__ rng) {
  const int k = threadIdx.x;
  if (k >= t.n) return;
  EntRec r;
  r.in_off = t.in_off[k];
  r.in_size = t.in_size[k];
  r.count = t.count[k];
  r.out_off = t.out_off[k];
  r.L = 0;
  r.valid = 0;
  unsigned long long S = 0;
  if (r.in_size >= HDR) {
    const uint8_t* p = blob + r.in_off;
    uint32_t L = 0;
    unsigned long long n = 0;
    for (int b = 0; b < 4; ++b) L |= (uint32_t)p[8 + b] << (8 * b);
    for (int b = 0; b < 8; ++b) n |= (unsigned long long)p[12 + b] << (8 * b);
    bool ok = p[0] == 'T' && p[1] == 'I' && p[2] == 'C' && p[3] == 'S' && p[4] == (HDR == 36 ? 3 : HDR == 28 ? 2 : 1) && !p[5] &&
              !p[6] && !p[7];
    if (HDR >= 28) {
      uint32_t hk = 0, hc = 0;
      for (int b = 0; b < 4; ++b) {
        hk |= (uint32_t)p[20 + b] << (8 * b);
        hc |= (uint32_t)p[24 + b] << (8 * b);
      }
      ok = ok && hk == K && hc == crc;
    }
    if (HDR == 36) {
      uint32_t h0 = 0, h1 = 0;
      for (int b = 0; b < 4; ++b) {
        h0 |= (uint32_t)p[28 + b] << (8 * b);
        h1 |= (uint32_t)p[32 + b] << (8 * b);
      }
      ok = ok && h0 == g0 && h1 == g1;
    }
    ok = ok && L >= 4 && L <= kEntMaxL && (L & 3) == 0 && n == (unsigned long long)r.count;
    if (ok) {
      S = (n + L - 1) / L;
      if (S > (unsigned long long)(r.in_size - HDR) / 2) ok = false;
    }
    if constexpr (RNG != 0) {
      const unsigned long long a = (unsigned long long)rg.first[k], c = (unsigned long long)rg.count[k];
      if (ok && (c == 0 || a >= n || c > n - a)) ok = false;
      if (ok) S = (a + c - 1) / L - a / L + 1;
    }
    if (ok) {
      r.L = L;
      r.valid = 1;
    } else {
      S = 0;
    }
  }
  rec[t.first + k] = r;
  seg_cnt[t.first + k] = S;
  if constexpr (RNG != 0) {
    EntRng q;
    q.first = rg.first[k];
    q.count = rg.count[k];
    rng[t.first + k] = q;
  }
}

// Workgroup i: the offsets of container i's payloads from its u16 lengths; a container that
// cannot be decoded (header, or its segments do not fit the scratch) becomes zeros.
// RNG: record i is a range; the scan still runs over segments 0 .. j1 of its container, to find
// the payload offsets, but keeps only those of j0 .. j1 (work item b + j - j0) and reads no length
// behind j1.  A range whose last payload would end outside the container becomes zeros too; only
// the range's own bytes of d_sym are ever written.
template <int HDR, int RNG>
__global__ void __launch_bounds__(256) ent_dec_scan_kernel(const uint8_t* __restrict__ blob, EntRec* __restrict__ rec,
                                                           const unsigned long long* __restrict__ seg_base,
                                                           unsigned long long cap,
                                                           unsigned long long* __restrict__ seg_off,
                                                           uint8_t* __restrict__ d_sym,
                                                           const EntRng* __restrict__ rng) {
  __shared__ unsigned long long s[256];
  const int i = blockIdx.x, t = threadIdx.x;
  const EntRec r = rec[i];
  const unsigned long long b = seg_base[i], S = seg_base[i + 1] - b;
  const long long fill = RNG ? rng[i].count : r.count;
  if (!r.valid || b + S > cap) {
    uint8_t* dst = d_sym + r.out_off;
    for (long long k = t; k < fill; k += 256) dst[k] = 0;
    if (t == 0) rec[i].valid = 0;
    return;
  }
  const uint8_t* lens = blob + r.in_off + HDR;
  // segments of the container; the first the record needs; one past the last it needs
  const unsigned long long Sc = RNG ? ((unsigned long long)r.count + r.L - 1) / r.L : S;
  const unsigned long long j0 = RNG ? (unsigned long long)rng[i].first / r.L : 0, je = j0 + S;
  unsigned long long carry = (unsigned long long)HDR + 2ull * Sc;
  for (unsigned long long jb = 0; jb < je; jb += 256) {
    const unsigned long long j = jb + t;
    const uint32_t len = j < je ? (uint32_t)lens[2 * j] | (uint32_t)lens[2 * j + 1] << 8 : 0;
    const unsigned long long inc = ent_block_scan(len, s);
    if (j < je && j >= j0) seg_off[b + j - j0] = carry + inc - len;
    carry += s[255];
    __syncthreads();
  }
  if (RNG && carry > (unsigned long long)r.in_size) {  // uniform: every thread holds the same carry
    uint8_t* dst = d_sym + r.out_off;
    for (long long k = t; k < fill; k += 256) dst[k] = 0;
    if (t == 0) rec[i].valid = 0;
  }
}

// One segment per lane, grid-stride.  Dynamic LDS: the cumulative table, then (lut != 0) the
// value -> symbol bytes.  The decode step has a second copy in ent_decode_ctx_kernel: a fix to the
// arithmetic goes into both.
// RNG (here and in the two decode kernels below): work item g of record i is segment j0 + (g -
// seg_base[i]) of the container.  The lane decodes it from its start, because the chain cannot
// begin in the middle, stops at the range's end and stores only symbols first <= k < first + count.
template <int RNG>
__global__ void __launch_bounds__(64) ent_decode_kernel(const EntModel m, int lut, const uint8_t* __restrict__ blob,
                                                        const EntRec* __restrict__ rec,
                                                        const unsigned long long* __restrict__ seg_base, int n_streams,
                                                        const unsigned long long* __restrict__ seg_off,
                                                        uint8_t* __restrict__ d_sym,
                                                        const EntRng* __restrict__ rng) {
  extern __shared__ uint32_t s_dyn[];
  uint32_t* s_cum = s_dyn;
  uint8_t* s_lut = reinterpret_cast<uint8_t*>(s_dyn + 260);
  const unsigned long long T = seg_base[n_streams];
  if ((unsigned long long)blockIdx.x * 64 >= T) return;
  const int nsym = m.nsym;
  const uint32_t total = m.cum[nsym];
  for (int k = threadIdx.x; k <= nsym; k += 64) s_cum[k] = m.cum[k];
  __syncthreads();
  auto search = [&](uint32_t val) {  // last s with cum[s] <= val
    int lo = 0, hi = nsym - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (s_cum[mid] <= val) lo = mid;
      else hi = mid - 1;
    }
    return (uint32_t)lo;
  };
  if (lut) {
    for (uint32_t v = threadIdx.x; v < total; v += 64) s_lut[v] = (uint8_t)search(v);
    __syncthreads();
  }
  const int shift = m.shift;

  for (unsigned long long g = (unsigned long long)blockIdx.x * 64 + threadIdx.x; g < T;
       g += (unsigned long long)gridDim.x * 64) {
    const int i = ent_find(seg_base, n_streams, g);
    const EntRec r = rec[i];
    if (!r.valid) continue;
    unsigned long long j = g - seg_base[i];
    if constexpr (RNG != 0) j += (unsigned long long)rng[i].first / r.L;
    const long long left = r.count - (long long)(j * r.L);
    uint32_t cnt = left < (long long)r.L ? (uint32_t)left : r.L;
    const uint8_t* cont = blob + r.in_off;
    const uint32_t len = (uint32_t)cont[20 + 2 * j] | (uint32_t)cont[20 + 2 * j + 1] << 8;
    // the segment's extent, clamped to the container
    const unsigned long long size = (unsigned long long)r.in_size;
    unsigned long long pos = seg_off[g];
    if (pos > size) pos = size;
    unsigned long long end = pos + len;
    if (end > size) end = size;
    uint8_t* dst = d_sym + r.out_off + (long long)(j * r.L);
    uint32_t lo = 0;  // the first symbol of the segment that is stored
    if constexpr (RNG != 0) {
      const long long first = rng[i].first, b = (long long)(j * r.L), stop = first + rng[i].count - b;
      if (stop < (long long)cnt) cnt = (uint32_t)stop;
      if (first > b) lo = (uint32_t)(first - b);
      dst = d_sym + (r.out_off + b - first);  // dst[k] is touched for k >= lo only
    }

    auto get = [&]() -> uint32_t { return pos < end ? (uint32_t)cont[pos++] : 0u; };
    uint32_t code = 0;
    for (int q = 0; q < 4; ++q) code = (code << 8) | get();
    unsigned long long range = 1ull << 32;
    auto dec = [&]() -> uint32_t {
      unsigned long long rr;
      if (shift >= 0) rr = range >> shift;
      else if (range >> 32) rr = range / total;
      else rr = (uint32_t)range / total;
      uint32_t val = (rr >> 32) ? 0u : code / (uint32_t)rr;
      if (val >= total) val = total - 1;
      const uint32_t s = lut ? (uint32_t)s_lut[val] : search(val);
      const uint32_t start = s_cum[s], next = s_cum[s + 1];
      const unsigned long long sr = (unsigned long long)start * rr;
      code -= (uint32_t)sr;
      range = next == total ? range - sr : (unsigned long long)(next - start) * rr;
      while (range < (1ull << 24)) {
        range <<= 8;
        code = (code << 8) | get();
      }
      return s;
    };

    uint32_t k = 0;
    for (; k < lo; ++k) (void)dec();  // RNG: in front of the range
    for (; k < cnt && ((uintptr_t)(dst + k) & 3) != 0; ++k) dst[k] = (uint8_t)dec();
    for (; k + 4 <= cnt; k += 4) {
      uint32_t w = 0;
#pragma unroll 1
      for (int b = 0; b < 4; ++b) w |= dec() << (8 * b);
      *reinterpret_cast<uint32_t*>(dst + k) = w;
    }
    for (; k < cnt; ++k) dst[k] = (uint8_t)dec();
  }
}

// --- version 2: K tables, symbol k of a stream under table k mod K ---
//
// The tables lie in a device buffer of the handle (tic_entropy_set_tables), K rows of ncum words:
// cum[1] .. cum[ncum - 1] (cum[0] is 0 by contract, so it is not stored; the last of them is the
// row's total), then the row's shift (log2 of the total, or -1).  LDS != 0: every workgroup copies
// them into dynamic LDS first (K * ncum * 4 <= 64 KiB); else the lanes read them from global
// memory, where the rows of neighbouring lanes' contexts share cache lines.  A lane carries its
// context as the word offset of its row, advanced by ncum per symbol and wrapped at K * ncum.
// The coder arithmetic is that of ent_encode_kernel / ent_decode_kernel, which keep their own
// copy (the table by value, one total) as they were measured: put / emit_top / the flush and the
// decoder's renormalisation exist twice, and a fix to either goes into both copies.

template <int LDS>
__global__ void __launch_bounds__(64) ent_encode_ctx_kernel(const uint32_t* __restrict__ g_tab, uint32_t K,
                                                            uint32_t ncum, const uint8_t* __restrict__ sym,
                                                            const EntRec* __restrict__ rec,
                                                            const unsigned long long* __restrict__ seg_base,
                                                            int n_streams, uint32_t L, uint8_t* __restrict__ slots,
                                                            uint32_t* __restrict__ seg_len) {
  extern __shared__ uint32_t s_dyn[];
  const uint32_t words = K * ncum;
  if (LDS) {
    for (uint32_t k = threadIdx.x; k < words; k += 64) s_dyn[k] = g_tab[k];
    __syncthreads();
  }
  auto tab = [&](uint32_t k) -> uint32_t { return LDS ? s_dyn[k] : g_tab[k]; };
  const unsigned long long T = seg_base[n_streams];
  const unsigned long long g = (unsigned long long)blockIdx.x * 64 + threadIdx.x;
  if (g >= T) return;
  const int i = ent_find(seg_base, n_streams, g);
  const unsigned long long j = g - seg_base[i];
  const long long left = rec[i].count - (long long)(j * L);
  const uint32_t cnt = left < (long long)L ? (uint32_t)left : L;
  const uint8_t* src = sym + rec[i].in_off + (long long)(j * L);
  uint32_t* out = reinterpret_cast<uint32_t*>(slots + (size_t)g * ent_stride(L));

  const uint32_t nsym = ncum - 1;
  uint32_t row = (uint32_t)((j * L) % K) * ncum;  // every stream starts at context 0
  unsigned long long low = 0, range = 1ull << 32;
  int cache = -1;
  uint32_t pending = 0, nout = 0, acc = 0;
  bool bad = false;

  auto put = [&](uint32_t b) {
    acc |= (b & 0xFFu) << (8 * (nout & 3));
    ++nout;
    if ((nout & 3) == 0) {
      out[(nout >> 2) - 1] = acc;
      acc = 0;
    }
  };
  auto emit_top = [&]() {
    if (low < 0xFF000000ull || low >= (1ull << 32)) {
      const uint32_t carry = low >= (1ull << 32) ? 1u : 0u;
      if (cache >= 0) put((uint32_t)cache + carry);
      for (; pending; --pending) put(0xFFu + carry);
      cache = (int)((low >> 24) & 0xFF);
    } else {
      ++pending;
    }
    low = (low << 8) & 0xFFFFFFFFull;
  };
  auto step = [&](uint32_t s) {
    const uint32_t at = row;
    row += ncum;
    if (row == words) row = 0;
    if (s >= nsym) {
      bad = true;
      return;
    }
    const uint32_t start = s ? tab(at + s - 1) : 0u, next = tab(at + s), total = tab(at + nsym - 1);
    const int shift = (int)tab(at + nsym);
    unsigned long long r;
    if (shift >= 0) r = range >> shift;
    else if (range >> 32) r = range / total;
    else r = (uint32_t)range / total;
    const unsigned long long sr = (unsigned long long)start * r;
    low += sr;
    range = next == total ? range - sr : (unsigned long long)(next - start) * r;
    while (range < (1ull << 24)) {
      range <<= 8;
      emit_top();
    }
  };

  uint32_t k = 0;
  for (; k < cnt && ((uintptr_t)(src + k) & 15) != 0; ++k) step(src[k]);
  for (; k + 16 <= cnt; k += 16) {
    const uint4 v = *reinterpret_cast<const uint4*>(src + k);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t x = w[q];
#pragma unroll 1
      for (int b = 0; b < 4; ++b) {
        step(x & 0xFFu);
        x >>= 8;
      }
    }
  }
  for (; k < cnt; ++k) step(src[k]);

  // the minimal flush (range_coder.cpp EncCore::finish)
  int nb = 0;
  unsigned long long v = low;
  for (; nb <= 4; ++nb) {
    if (nb == 4) {
      v = low;
    } else {
      const unsigned long long unit = 1ull << (32 - 8 * nb);
      v = (low + unit - 1) & ~(unit - 1);
    }
    if (v < low + range) break;
  }
  low = v;
  for (int q = 0; q < nb; ++q) emit_top();
  if (nb > 0) {
    if (cache >= 0) put((uint32_t)cache);
    for (; pending; --pending) put(0xFFu);
  } else if (cache >= 0) {
    const uint32_t carry = v >= (1ull << 32) ? 1u : 0u;
    put((uint32_t)cache + carry);
    for (; pending; --pending) put(0xFFu + carry);
  }
  if (nout & 3) out[nout >> 2] = acc;  // the slot is a multiple of 4 bytes
  seg_len[g] = bad ? kEntBad : nout;
}

// One segment per lane, grid-stride.  No value -> symbol bytes: with two symbols (ncum == 3, the
// shipped models) the symbol is one compare with cum[1], otherwise the host's binary search.
template <int LDS, int RNG>
__global__ void __launch_bounds__(64) ent_decode_ctx_kernel(const uint32_t* __restrict__ g_tab, uint32_t K,
                                                            uint32_t ncum, const uint8_t* __restrict__ blob,
                                                            const EntRec* __restrict__ rec,
                                                            const unsigned long long* __restrict__ seg_base,
                                                            int n_streams,
                                                            const unsigned long long* __restrict__ seg_off,
                                                            uint8_t* __restrict__ d_sym,
                                                            const EntRng* __restrict__ rng) {
  extern __shared__ uint32_t s_dyn[];
  const unsigned long long T = seg_base[n_streams];
  if ((unsigned long long)blockIdx.x * 64 >= T) return;
  const uint32_t words = K * ncum;
  if (LDS) {
    for (uint32_t k = threadIdx.x; k < words; k += 64) s_dyn[k] = g_tab[k];
    __syncthreads();
  }
  auto tab = [&](uint32_t k) -> uint32_t { return LDS ? s_dyn[k] : g_tab[k]; };
  const uint32_t nsym = ncum - 1;
  const bool two = ncum == 3;

  for (unsigned long long g = (unsigned long long)blockIdx.x * 64 + threadIdx.x; g < T;
       g += (unsigned long long)gridDim.x * 64) {
    const int i = ent_find(seg_base, n_streams, g);
    const EntRec r = rec[i];
    if (!r.valid) continue;
    unsigned long long j = g - seg_base[i];
    if constexpr (RNG != 0) j += (unsigned long long)rng[i].first / r.L;
    const long long left = r.count - (long long)(j * r.L);
    uint32_t cnt = left < (long long)r.L ? (uint32_t)left : r.L;
    const uint8_t* cont = blob + r.in_off;
    const uint32_t len = (uint32_t)cont[28 + 2 * j] | (uint32_t)cont[28 + 2 * j + 1] << 8;
    // the segment's extent, clamped to the container
    const unsigned long long size = (unsigned long long)r.in_size;
    unsigned long long pos = seg_off[g];
    if (pos > size) pos = size;
    unsigned long long end = pos + len;
    if (end > size) end = size;
    uint8_t* dst = d_sym + r.out_off + (long long)(j * r.L);
    uint32_t lo = 0;  // the first symbol of the segment that is stored
    if constexpr (RNG != 0) {
      const long long first = rng[i].first, b = (long long)(j * r.L), stop = first + rng[i].count - b;
      if (stop < (long long)cnt) cnt = (uint32_t)stop;
      if (first > b) lo = (uint32_t)(first - b);
      dst = d_sym + (r.out_off + b - first);  // dst[k] is touched for k >= lo only
    }
    uint32_t row = (uint32_t)((j * r.L) % K) * ncum;

    auto get = [&]() -> uint32_t { return pos < end ? (uint32_t)cont[pos++] : 0u; };
    uint32_t code = 0;
    for (int q = 0; q < 4; ++q) code = (code << 8) | get();
    unsigned long long range = 1ull << 32;
    auto dec = [&]() -> uint32_t {
      const uint32_t at = row;
      row += ncum;
      if (row == words) row = 0;
      const uint32_t total = tab(at + nsym - 1);
      const int shift = (int)tab(at + nsym);
      unsigned long long rr;
      if (shift >= 0) rr = range >> shift;
      else if (range >> 32) rr = range / total;
      else rr = (uint32_t)range / total;
      uint32_t val = (rr >> 32) ? 0u : code / (uint32_t)rr;
      if (val >= total) val = total - 1;
      uint32_t s, start, next;
      if (two) {
        const uint32_t c1 = tab(at);
        s = val >= c1 ? 1u : 0u;
        start = s ? c1 : 0u;
        next = s ? total : c1;
      } else {
        uint32_t lo = 0, hi = nsym - 1;  // last s with cum[s] <= val; cum[mid] is word mid - 1, mid >= 1
        while (lo < hi) {
          const uint32_t mid = (lo + hi + 1) >> 1;
          if (tab(at + mid - 1) <= val) lo = mid;
          else hi = mid - 1;
        }
        s = lo;
        start = s ? tab(at + s - 1) : 0u;
        next = tab(at + s);
      }
      const unsigned long long sr = (unsigned long long)start * rr;
      code -= (uint32_t)sr;
      range = next == total ? range - sr : (unsigned long long)(next - start) * rr;
      while (range < (1ull << 24)) {
        range <<= 8;
        code = (code << 8) | get();
      }
      return s;
    };

    uint32_t k = 0;
    for (; k < lo; ++k) (void)dec();  // RNG: in front of the range
    for (; k < cnt && ((uintptr_t)(dst + k) & 3) != 0; ++k) dst[k] = (uint8_t)dec();
    for (; k + 4 <= cnt; k += 4) {
      uint32_t w = 0;
#pragma unroll 1
      for (int b = 0; b < 4; ++b) w |= dec() << (8 * b);
      *reinterpret_cast<uint32_t*>(dst + k) = w;
    }
    for (; k < cnt; ++k) dst[k] = (uint8_t)dec();
  }
}

// Thread x: one context c (consecutive lanes read consecutive bytes); blockIdx.y strides over the
// rows of K symbols.  np.histogram semantics as histogram_kernel (v == Q counts in the last bin,
// larger values in none).  A lane adds a run of equal symbols with one 64-bit atomic: channels
// are biased, so runs are long.  Integer adds: the sums do not depend on their order.
__global__ void __launch_bounds__(256) ent_histogram_ctx_kernel(const uint8_t* __restrict__ sym, size_t n, int Q,
                                                                uint32_t K, unsigned long long* __restrict__ counts) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c >= K) return;
  unsigned long long* mine = counts + (size_t)c * Q;
  uint32_t cur = 0, run = 0;
  for (size_t at = (size_t)blockIdx.y * K + c; at < n; at += (size_t)gridDim.y * K) {
    uint32_t v = sym[at];
    if (v == (uint32_t)Q) v = Q - 1;
    if (v >= (uint32_t)Q) continue;
    if (v != cur && run) {
      atomicAdd(&mine[cur], (unsigned long long)run);
      run = 0;
    }
    cur = v;
    ++run;
  }
  if (run) atomicAdd(&mine[cur], (unsigned long long)run);
}

// --- version 3: K0 periodic contexts x the classes of the causal neighbours (include/tic.h) ---
//
// The tables lie in the handle's buffer in version 2's layout, K0 * M rows; symbol k's row is
// (k mod K0) * M + nb.  A lane carries its place in the code as counters that wrap: (c, w, h) and
// the word offset of its K0 phase, advanced by M * ncum per symbol; the one division is at the
// start of a segment.  A neighbour counts only inside the lane's own segment (k - C >= 0 or
// k - ew*C >= 0 in segment-local k), so no lane needs another lane's symbols.
//   encoder  reads the neighbours' symbols from its input, off the low / range chain
//   decoder  RING: the classes of the lane's last `ring` symbols are a ring of bits in LDS (word i
//            of lane l at [i * 64 + l]: lanes never share a bank).  ring is the distance of the
//            farthest neighbour a segment can reach (ew*C, or C when neighbours = 1 or ew*C is
//            not below the longest segment), so the bit about to be overwritten is that
//            neighbour's and the W bit lies C behind it.  The word under the write position is
//            held in a register and goes back to LDS when the position leaves it.  Bits of an
//            earlier segment are never used: the validity tests come first.
//            !RING (the rings of a workgroup over 64 KiB): every symbol is stored as a byte at
//            once and the lane re-reads the bytes it stored itself.
// The coder arithmetic is a third copy of ent_encode_kernel's / ent_decode_kernel's (the measured
// kernels stay as they are): a fix to the carry, flush or renormalisation goes into all three.
struct EntNbr {
  uint32_t K0, M, ncum, two;   // two: the N neighbour counts (neighbours = 2)
  uint32_t eh, ew, C, rowC;    // rowC = ew * C (below 2^32: each at most 65535)
  uint32_t ring;               // decoder: bits of a lane's ring (0: no neighbour lies inside any segment)
};

struct EntNbrPos {
  uint32_t c, w, h, row;  // row: word offset of table row (k mod K0) * M
  __device__ __forceinline__ void start(const EntNbr& q, unsigned long long o) {
    const unsigned long long p = o % ((unsigned long long)q.eh * q.rowC);
    h = (uint32_t)(p / q.rowC);
    const uint32_t r = (uint32_t)(p - (unsigned long long)h * q.rowC);
    w = r / q.C;
    c = r - w * q.C;
    row = (uint32_t)(o % q.K0) * q.M * q.ncum;
  }
  __device__ __forceinline__ void advance(const EntNbr& q, uint32_t words) {
    row += q.M * q.ncum;
    if (row == words) row = 0;
    if (++c == q.C) {
      c = 0;
      if (++w == q.ew) {
        w = 0;
        if (++h == q.eh) h = 0;
      }
    }
  }
};

template <int LDS>
__global__ void __launch_bounds__(64) ent_encode_nbr_kernel(const uint32_t* __restrict__ g_tab, const EntNbr q,
                                                            const uint8_t* __restrict__ sym,
                                                            const EntRec* __restrict__ rec,
                                                            const unsigned long long* __restrict__ seg_base,
                                                            int n_streams, uint32_t L, uint8_t* __restrict__ slots,
                                                            uint32_t* __restrict__ seg_len) {
  extern __shared__ uint32_t s_dyn[];
  const uint32_t ncum = q.ncum, words = q.K0 * q.M * ncum;
  if (LDS) {
    for (uint32_t k = threadIdx.x; k < words; k += 64) s_dyn[k] = g_tab[k];
    __syncthreads();
  }
  auto tab = [&](uint32_t k) -> uint32_t { return LDS ? s_dyn[k] : g_tab[k]; };
  const unsigned long long T = seg_base[n_streams];
  const unsigned long long g = (unsigned long long)blockIdx.x * 64 + threadIdx.x;
  if (g >= T) return;
  const int i = ent_find(seg_base, n_streams, g);
  const unsigned long long j = g - seg_base[i];
  const long long left = rec[i].count - (long long)(j * L);
  const uint32_t cnt = left < (long long)L ? (uint32_t)left : L;
  const uint8_t* src = sym + rec[i].in_off + (long long)(j * L);
  uint32_t* out = reinterpret_cast<uint32_t*>(slots + (size_t)g * ent_stride(L));

  const uint32_t nsym = ncum - 1;
  EntNbrPos at;
  at.start(q, j * L);  // every stream starts at position 0 of a patch
  unsigned long long low = 0, range = 1ull << 32;
  int cache = -1;
  uint32_t pending = 0, nout = 0, acc = 0;
  bool bad = false;

  auto put = [&](uint32_t b) {
    acc |= (b & 0xFFu) << (8 * (nout & 3));
    ++nout;
    if ((nout & 3) == 0) {
      out[(nout >> 2) - 1] = acc;
      acc = 0;
    }
  };
  auto emit_top = [&]() {
    if (low < 0xFF000000ull || low >= (1ull << 32)) {
      const uint32_t carry = low >= (1ull << 32) ? 1u : 0u;
      if (cache >= 0) put((uint32_t)cache + carry);
      for (; pending; --pending) put(0xFFu + carry);
      cache = (int)((low >> 24) & 0xFF);
    } else {
      ++pending;
    }
    low = (low << 8) & 0xFFFFFFFFull;
  };
  // symbol s at segment-local index k; clsW, clsN: the classes of the symbols at k - C and k - ew*C
  // (read only where that index lies inside the segment)
  auto step = [&](uint32_t k, uint32_t s, uint32_t clsW, uint32_t clsN) {
    uint32_t nb = 0;
    if (at.w && k >= q.C) nb = 1u + clsW;
    if (q.two && at.h && k >= q.rowC) nb += 3u * (1u + clsN);
    const uint32_t r0 = at.row + nb * ncum;
    at.advance(q, words);
    if (s >= nsym) {
      bad = true;
      return;
    }
    const uint32_t start = s ? tab(r0 + s - 1) : 0u, next = tab(r0 + s), total = tab(r0 + nsym - 1);
    const int shift = (int)tab(r0 + nsym);
    unsigned long long r;
    if (shift >= 0) r = range >> shift;
    else if (range >> 32) r = range / total;
    else r = (uint32_t)range / total;
    const unsigned long long sr = (unsigned long long)start * r;
    low += sr;
    range = next == total ? range - sr : (unsigned long long)(next - start) * r;
    while (range < (1ull << 24)) {
      range <<= 8;
      emit_top();
    }
  };

  auto cls = [&](uint32_t j) -> uint32_t { return 2u * src[j] >= nsym ? 1u : 0u; };
  auto one = [&](uint32_t k) {
    step(k, src[k], k >= q.C ? cls(k - q.C) : 0u, q.two && k >= q.rowC ? cls(k - q.rowC) : 0u);
  };
  uint32_t k = 0;
  for (; k < cnt && ((uintptr_t)(src + k) & 15) != 0; ++k) one(k);
  for (; k + 16 <= cnt; k += 16) {
    const uint4 v = *reinterpret_cast<const uint4*>(src + k);
    // the block's 16 + 16 neighbour classes as bit masks: independent loads, all in flight before
    // the chain of 16 symbols starts, instead of two loads inside every step
    uint32_t mW = 0, mN = 0;
    if (k + 15 >= q.C) {
#pragma unroll
      for (int b = 0; b < 16; ++b)
        if (k + b >= q.C) mW |= cls(k + b - q.C) << b;
    }
    if (q.two && k + 15 >= q.rowC) {
#pragma unroll
      for (int b = 0; b < 16; ++b)
        if (k + b >= q.rowC) mN |= cls(k + b - q.rowC) << b;
    }
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      uint32_t x = w[qq];
#pragma unroll 1
      for (int b = 0; b < 4; ++b) {
        step(k + 4 * qq + b, x & 0xFFu, mW & 1u, mN & 1u);
        x >>= 8;
        mW >>= 1;
        mN >>= 1;
      }
    }
  }
  for (; k < cnt; ++k) one(k);

  // the minimal flush (range_coder.cpp EncCore::finish)
  int nb = 0;
  unsigned long long v = low;
  for (; nb <= 4; ++nb) {
    if (nb == 4) {
      v = low;
    } else {
      const unsigned long long unit = 1ull << (32 - 8 * nb);
      v = (low + unit - 1) & ~(unit - 1);
    }
    if (v < low + range) break;
  }
  low = v;
  for (int qq = 0; qq < nb; ++qq) emit_top();
  if (nb > 0) {
    if (cache >= 0) put((uint32_t)cache);
    for (; pending; --pending) put(0xFFu);
  } else if (cache >= 0) {
    const uint32_t carry = v >= (1ull << 32) ? 1u : 0u;
    put((uint32_t)cache + carry);
    for (; pending; --pending) put(0xFFu + carry);
  }
  if (nout & 3) out[nout >> 2] = acc;  // the slot is a multiple of 4 bytes
  seg_len[g] = bad ? kEntBad : nout;
}

// One segment per lane, grid-stride.  Dynamic LDS: the tables (LDS), then the rings (RING).
// d_sym is not __restrict__: with !RING a lane loads bytes it stored.
// RNG: a lane does not store the symbols in front of its range, so it cannot re-read them: where
// the rings of 64 lanes exceed 64 KiB (!RING), 32 lanes of the workgroup work (LN), each with its
// ring in LDS (at most 16383 bits, 2 KiB), and the other 32 only help to stage the tables.
template <int LDS, int RING, int RNG>
__global__ void __launch_bounds__(64) ent_decode_nbr_kernel(const uint32_t* __restrict__ g_tab, const EntNbr q,
                                                            const uint8_t* __restrict__ blob,
                                                            const EntRec* __restrict__ rec,
                                                            const unsigned long long* __restrict__ seg_base,
                                                            int n_streams,
                                                            const unsigned long long* __restrict__ seg_off,
                                                            uint8_t* d_sym, const EntRng* __restrict__ rng) {
  constexpr int LN = (RNG != 0 && !RING) ? 32 : 64;  // working lanes; ring words of a lane lie LN apart
  constexpr bool kRing = RING || RNG != 0;
  extern __shared__ uint32_t s_dyn[];
  const unsigned long long T = seg_base[n_streams];
  if ((unsigned long long)blockIdx.x * LN >= T) return;
  const uint32_t ncum = q.ncum, words = q.K0 * q.M * ncum;
  if (LDS) {
    for (uint32_t k = threadIdx.x; k < words; k += 64) s_dyn[k] = g_tab[k];
    __syncthreads();
  }
  auto tab = [&](uint32_t k) -> uint32_t { return LDS ? s_dyn[k] : g_tab[k]; };
  if (LN < 64 && threadIdx.x >= LN) return;  // behind the barrier above
  uint32_t* ring = s_dyn + (LDS ? words : 0) + threadIdx.x;  // this lane's words, LN apart
  const uint32_t R = q.ring;
  const bool useN = q.two && q.rowC == R;  // else no segment reaches its N neighbour
  const uint32_t nsym = ncum - 1;
  const bool two = ncum == 3;

  for (unsigned long long g = (unsigned long long)blockIdx.x * LN + threadIdx.x; g < T;
       g += (unsigned long long)gridDim.x * LN) {
    const int i = ent_find(seg_base, n_streams, g);
    const EntRec r = rec[i];
    if (!r.valid) continue;
    unsigned long long j = g - seg_base[i];
    if constexpr (RNG != 0) j += (unsigned long long)rng[i].first / r.L;
    const long long left = r.count - (long long)(j * r.L);
    uint32_t cnt = left < (long long)r.L ? (uint32_t)left : r.L;
    const uint8_t* cont = blob + r.in_off;
    const uint32_t len = (uint32_t)cont[36 + 2 * j] | (uint32_t)cont[36 + 2 * j + 1] << 8;
    // the segment's extent, clamped to the container
    const unsigned long long size = (unsigned long long)r.in_size;
    unsigned long long pos = seg_off[g];
    if (pos > size) pos = size;
    unsigned long long end = pos + len;
    if (end > size) end = size;
    uint8_t* dst = d_sym + r.out_off + (long long)(j * r.L);
    uint32_t lo = 0;  // the first symbol of the segment that is stored
    if constexpr (RNG != 0) {
      const long long first = rng[i].first, b = (long long)(j * r.L), stop = first + rng[i].count - b;
      if (stop < (long long)cnt) cnt = (uint32_t)stop;
      if (first > b) lo = (uint32_t)(first - b);
      dst = d_sym + (r.out_off + b - first);  // dst[k] is touched for k >= lo only
    }
    EntNbrPos at;
    at.start(q, j * r.L);
    uint32_t rp = 0, rw = R ? (R - q.C % R) % R : 0;  // ring places of symbol k - R and of symbol k - C
    // the ring word that holds place rp, kept in a register and written back when rp leaves it
    uint32_t far = kRing && R ? ring[0] : 0u;

    auto get = [&]() -> uint32_t { return pos < end ? (uint32_t)cont[pos++] : 0u; };
    uint32_t code = 0;
    for (int b = 0; b < 4; ++b) code = (code << 8) | get();
    unsigned long long range = 1ull << 32;
    // symbol at segment-local index k
    auto dec = [&](uint32_t k) -> uint32_t {
      uint32_t nb = 0;
      if (kRing) {
        if (R) {
          // a place in the word under rp is read from the register: the word in LDS is older
          const uint32_t near = (rw >> 5) == (rp >> 5) ? far : ring[(rw >> 5) * LN];
          if (at.w && k >= q.C) nb = 1u + ((near >> (rw & 31)) & 1u);
          if (useN && at.h && k >= R) nb += 3u * (1u + ((far >> (rp & 31)) & 1u));
        }
      } else {
        if (at.w && k >= q.C) nb = 1u + (2u * dst[k - q.C] >= nsym ? 1u : 0u);
        if (q.two && at.h && k >= q.rowC) nb += 3u * (1u + (2u * dst[k - q.rowC] >= nsym ? 1u : 0u));
      }
      const uint32_t r0 = at.row + nb * ncum;
      at.advance(q, words);
      const uint32_t total = tab(r0 + nsym - 1);
      const int shift = (int)tab(r0 + nsym);
      unsigned long long rr;
      if (shift >= 0) rr = range >> shift;
      else if (range >> 32) rr = range / total;
      else rr = (uint32_t)range / total;
      uint32_t val = (rr >> 32) ? 0u : code / (uint32_t)rr;
      if (val >= total) val = total - 1;
      uint32_t s, start, next;
      if (two) {
        const uint32_t c1 = tab(r0);
        s = val >= c1 ? 1u : 0u;
        start = s ? c1 : 0u;
        next = s ? total : c1;
      } else {
        uint32_t lo = 0, hi = nsym - 1;  // last s with cum[s] <= val; cum[mid] is word mid - 1, mid >= 1
        while (lo < hi) {
          const uint32_t mid = (lo + hi + 1) >> 1;
          if (tab(r0 + mid - 1) <= val) lo = mid;
          else hi = mid - 1;
        }
        s = lo;
        start = s ? tab(r0 + s - 1) : 0u;
        next = tab(r0 + s);
      }
      const unsigned long long sr = (unsigned long long)start * rr;
      code -= (uint32_t)sr;
      range = next == total ? range - sr : (unsigned long long)(next - start) * rr;
      while (range < (1ull << 24)) {
        range <<= 8;
        code = (code << 8) | get();
      }
      if (kRing && R) {  // this symbol's class replaces that of symbol k - R
        const uint32_t bit = 1u << (rp & 31), word = rp >> 5;
        far = 2u * s >= nsym ? far | bit : far & ~bit;
        if (++rp == R) rp = 0;
        if (++rw == R) rw = 0;
        if ((rp >> 5) != word) {
          ring[word * LN] = far;
          far = ring[(rp >> 5) * LN];
        }
      }
      return s;
    };

    if (kRing) {
      uint32_t k = 0;
      for (; k < lo; ++k) (void)dec(k);  // RNG: in front of the range
      for (; k < cnt && ((uintptr_t)(dst + k) & 3) != 0; ++k) dst[k] = (uint8_t)dec(k);
      for (; k + 4 <= cnt; k += 4) {
        uint32_t w = 0;
#pragma unroll 1
        for (int b = 0; b < 4; ++b) w |= dec(k + b) << (8 * b);
        *reinterpret_cast<uint32_t*>(dst + k) = w;
      }
      for (; k < cnt; ++k) dst[k] = (uint8_t)dec(k);
    } else {
      for (uint32_t k = 0; k < cnt; ++k) dst[k] = (uint8_t)dec(k);
    }
  }
}

// blockIdx.y: stream t.first + y of the chunk.  A thread takes pieces of 64 symbols, none across a
// segment, finds its place once per piece and then walks the counters as the coders do.
// np.histogram semantics as histogram_kernel (v == Q counts in the last bin, larger values in
// none; a neighbour's class is that of its bin).  Integer adds: the sums do not depend on their order.
__global__ void __launch_bounds__(256) ent_histogram_nbr_kernel(const EntChunk t, const EntNbr q,
                                                                const uint8_t* __restrict__ sym, int Q, uint32_t L,
                                                                unsigned long long* __restrict__ counts) {
  const int i = blockIdx.y;
  if (i >= t.n) return;
  const unsigned long long n = (unsigned long long)t.count[i];
  const uint8_t* src = sym + t.in_off[i];
  const unsigned long long per = (L + 63) / 64, pieces = ((n + L - 1) / L) * per;
  const uint32_t uq = (uint32_t)Q, rows = q.K0 * q.M;
  auto bin = [&](uint32_t v) { return v >= uq ? uq - 1 : v; };
  for (unsigned long long pc = (unsigned long long)blockIdx.x * 256 + threadIdx.x; pc < pieces;
       pc += (unsigned long long)gridDim.x * 256) {
    const unsigned long long seg0 = (pc / per) * L, a = seg0 + (pc % per) * 64;
    unsigned long long e = a + 64;
    if (e > seg0 + L) e = seg0 + L;
    if (e > n) e = n;
    if (a >= e) continue;
    EntNbr rowsOnly = q;
    rowsOnly.ncum = 1;  // `row` then counts table rows, not words
    EntNbrPos at;
    at.start(rowsOnly, a);
    for (unsigned long long k = a; k < e; ++k) {
      uint32_t nb = 0;
      if (at.w && k - seg0 >= q.C) nb = 1u + (2u * bin(src[k - q.C]) >= uq ? 1u : 0u);
      if (q.two && at.h && k - seg0 >= q.rowC) nb += 3u * (1u + (2u * bin(src[k - q.rowC]) >= uq ? 1u : 0u));
      const uint32_t row = at.row + nb;
      at.advance(rowsOnly, rows);
      const uint32_t v = src[k];
      if (v <= uq) atomicAdd(&counts[(size_t)row * Q + bin(v)], 1ull);
    }
  }
}

}  // namespace tic

namespace {

// The version-2 tables of a handle on its device: K rows of ncum words (the layout above
// ent_encode_ctx_kernel), the CRC the containers carry.
struct EntTables {
  uint32_t* d_tab = nullptr;
  size_t cap_words = 0;
  uint32_t K = 0, ncum = 0, crc = 0;
  // version 3 (tic_entropy_set_tables_nbr; neighbours == 0: the tables are version 2's): K = K0 * M
  uint32_t K0 = 0, neighbours = 0, eh = 0, ew = 0, C = 0;
};
struct EntState {
  tic::EntModel m;
  bool has_m = false;
  EntTables t;
};
std::mutex g_ent_mu;
std::map<tic_handle*, EntState> g_ent;

// Bytes in front of the per-segment arrays: seg_base[n + 1], a second u64[n + 1] (container
// offsets / segment counts), the records.
size_t ent_fixed(int n) {
  const size_t b = 2 * ((size_t)n + 1) * 8 + (size_t)n * sizeof(tic::EntRec);
  return (b + 15) & ~(size_t)15;
}
bool ent_L_ok(uint32_t L) { return L >= 4 && L <= tic::kEntMaxL && L % 4 == 0; }

// Segments of the list at segment length L, or -1 for a bad count / more than 2^31 - 1.
long long ent_segments(const int64_t* counts, int n, uint32_t L, const char** why) {
  long long T = 0;
  for (int i = 0; i < n; ++i) {
    if (counts[i] <= 0) {
      *why = "every stream needs at least one symbol";
      return -1;
    }
    if (counts[i] > (1ll << 40)) {
      *why = "a stream of more than 2^40 symbols";
      return -1;
    }
    T += (counts[i] + L - 1) / L;
    if (T > INT_MAX) {
      *why = "more than 2^31 - 1 segments";
      return -1;
    }
  }
  return T;
}
size_t ent_scratch(int n, long long T, uint32_t L) {
  const size_t per = (((size_t)T * 12 + 15) & ~(size_t)15);  // seg_off u64, seg_len u32
  return ent_fixed(n) + per + (size_t)T * tic::ent_stride(L);
}

struct EntScratch {
  unsigned long long *seg_base, *aux, *seg_off;
  tic::EntRec* rec;
  uint32_t* seg_len;
  uint8_t* slots;
};
EntScratch ent_carve(void* d_scratch, int n, long long T) {
  EntScratch s;
  uint8_t* p = static_cast<uint8_t*>(d_scratch);
  s.seg_base = reinterpret_cast<unsigned long long*>(p);
  s.aux = s.seg_base + n + 1;
  s.rec = reinterpret_cast<tic::EntRec*>(s.aux + n + 1);
  p += ent_fixed(n);
  s.seg_off = reinterpret_cast<unsigned long long*>(p);
  s.seg_len = reinterpret_cast<uint32_t*>(s.seg_off + T);
  s.slots = p + (((size_t)T * 12 + 15) & ~(size_t)15);
  return s;
}

int ent_model(tic_handle* h, tic::EntModel* m) {
  std::lock_guard<std::mutex> lk(g_ent_mu);
  auto it = g_ent.find(h);
  if (it == g_ent.end() || !it->second.has_m)
    return fail(TIC_EINVAL, "no entropy table set on this handle (tic_entropy_set_table)");
  *m = it->second.m;
  return TIC_OK;
}

int ent_tables(tic_handle* h, EntTables* t, bool nbr = false) {
  std::lock_guard<std::mutex> lk(g_ent_mu);
  auto it = g_ent.find(h);
  const bool have = it != g_ent.end() && it->second.t.d_tab && it->second.t.K;
  if (nbr && (!have || !it->second.t.neighbours))
    return fail(TIC_EINVAL, "no neighbour tables set on this handle (tic_entropy_set_tables_nbr)");
  if (!nbr && (!have || it->second.t.neighbours))
    return fail(TIC_EINVAL, "no context tables set on this handle (tic_entropy_set_tables)");
  *t = it->second.t;
  return TIC_OK;
}

// The kernels' view of version-3 tables; ring: the farthest neighbour a segment can reach.
tic::EntNbr ent_nbr(const EntTables& t) {
  tic::EntNbr q;
  q.K0 = t.K0;
  q.M = t.neighbours == 2 ? 9 : 3;
  q.ncum = t.ncum;
  q.two = t.neighbours == 2;
  q.eh = t.eh, q.ew = t.ew, q.C = t.C;
  q.rowC = t.ew * t.C;
  q.ring = q.two && q.rowC < tic::kEntMaxL ? q.rowC : (q.C < tic::kEntMaxL ? q.C : 0);
  return q;
}

constexpr size_t kEntLdsTables = 64 * 1024;  // tables up to this many bytes are staged in LDS
constexpr size_t kEntLdsRings = 64 * 1024;   // a workgroup's class rings up to this many bytes live in LDS

// Both coders' launches differ between the versions only in the header size, the table's source
// and the coder kernel: ver is the container version.
int ent_encode(tic_handle* h, const uint8_t* d_sym, const int64_t* sym_offsets, const int64_t* counts, int n_streams,
               uint32_t L, void* d_scratch, size_t scratch_bytes, uint8_t* d_out, size_t out_cap, uint64_t* d_sizes,
               int ver);
int ent_decode(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets, const int64_t* blob_sizes,
               const int64_t* counts, int n_streams, uint8_t* d_sym, const int64_t* sym_offsets, void* d_scratch,
               size_t scratch_bytes, int ver);
// The same for one symbol range [firsts[r], firsts[r] + rcounts[r]) per record; counts: the
// containers' n.
int ent_decode_ranges(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets, const int64_t* blob_sizes,
                      const int64_t* counts, const int64_t* firsts, const int64_t* rcounts, int n_ranges,
                      uint8_t* d_sym, const int64_t* sym_offsets, void* d_scratch, size_t scratch_bytes, int ver);
// Most segments a range of `count` symbols touches at segment length L, wherever it starts; no
// larger at any longer L.
long long ent_range_segments(long long count, uint32_t L) { return (count + L - 2) / L + 1; }
int ent_upload_tables(tic_handle* h, const int64_t* tables, size_t K, size_t ncum, EntTables meta);

}  // namespace

extern "C" {

void tic_destroy_runtime_(tic_handle* h);

void tic_destroy(tic_handle* h) {
  if (h) {
    std::lock_guard<std::mutex> lk(g_ent_mu);
    auto it = g_ent.find(h);
    if (it != g_ent.end()) {
      if (it->second.t.d_tab && hipSetDevice(h->device) == hipSuccess) (void)hipFree(it->second.t.d_tab);
      g_ent.erase(it);
    }
  }
  tic_destroy_runtime_(h);
}

int tic_entropy_set_table(tic_handle* h, const int64_t* cum, size_t ncum) {
  if (!h) return fail(TIC_EINVAL, "null handle");
  // the host coder's own table check: one symbol through tic_rcseg_encode
  const uint8_t zero = 0;
  uint8_t out[32];
  size_t w = 0;
  const int rc = tic_rcseg_encode(&zero, 1, 4, cum, ncum, out, sizeof(out), &w);
  if (rc) return fail(rc, "%s", tic_rc_last_error());
  EntState st;
  memset(&st, 0, sizeof(st));
  st.m.nsym = (int)ncum - 1;
  for (size_t i = 0; i < ncum; ++i) st.m.cum[i] = (uint32_t)cum[i];
  const uint32_t total = st.m.cum[ncum - 1];
  st.m.shift = -1;
  if ((total & (total - 1)) == 0)
    for (int s = 0; s <= 24; ++s)
      if ((1u << s) == total) st.m.shift = s;
  std::lock_guard<std::mutex> lk(g_ent_mu);
  EntState& cur = g_ent[h];
  cur.m = st.m;
  cur.has_m = true;
  return TIC_OK;
}

int tic_entropy_set_tables(tic_handle* h, const int64_t* tables, size_t K, size_t ncum) {
  if (!h) return fail(TIC_EINVAL, "null handle");
  // the host coder's own check of the tables, and their CRC: one symbol through tic_rcseg_encode_ctx
  const uint8_t zero = 0;
  uint8_t out[64];
  size_t w = 0;
  const int rc = tic_rcseg_encode_ctx(&zero, 1, 4, tables, K, ncum, out, sizeof(out), &w);
  if (rc) return fail(rc, "%s", tic_rc_last_error());
  EntTables meta;
  for (int b = 0; b < 4; ++b) meta.crc |= (uint32_t)out[24 + b] << (8 * b);
  return ent_upload_tables(h, tables, K, ncum, meta);
}

int tic_entropy_set_tables_nbr(tic_handle* h, const int64_t* tables, size_t K0, uint32_t neighbours, size_t ncum,
                               uint32_t eh, uint32_t ew, uint32_t C) {
  if (!h) return fail(TIC_EINVAL, "null handle");
  // the host coder's own check of the tables and the geometry, and the CRC: one symbol through
  // tic_rcseg_encode_nbr
  const uint8_t zero = 0;
  uint8_t out[64];
  size_t w = 0;
  const int rc = tic_rcseg_encode_nbr(&zero, 1, 4, tables, K0, neighbours, ncum, eh, ew, C, out, sizeof(out), &w);
  if (rc) return fail(rc, "%s", tic_rc_last_error());
  EntTables meta;
  for (int b = 0; b < 4; ++b) meta.crc |= (uint32_t)out[24 + b] << (8 * b);
  meta.K0 = (uint32_t)K0;
  meta.neighbours = neighbours;
  meta.eh = eh, meta.ew = ew, meta.C = C;
  return ent_upload_tables(h, tables, K0 * (neighbours == 2 ? 9 : 3), ncum, meta);
}

}  // extern "C"

namespace {
// Validated tables into the handle's device buffer, K rows in the coder kernels' layout; meta: the
// CRC and, version 3, what else the containers carry.
int ent_upload_tables(tic_handle* h, const int64_t* tables, size_t K, size_t ncum, EntTables meta) {
  const size_t words = K * ncum;
  std::vector<uint32_t> host(words);
  for (size_t k = 0; k < K; ++k) {
    const int64_t* cum = tables + k * ncum;
    uint32_t* row = host.data() + k * ncum;
    for (size_t s = 1; s < ncum; ++s) row[s - 1] = (uint32_t)cum[s];
    const uint32_t total = (uint32_t)cum[ncum - 1];
    int shift = -1;
    if ((total & (total - 1)) == 0)
      for (int q = 0; q <= 24; ++q)
        if ((1u << q) == total) shift = q;
    row[ncum - 1] = (uint32_t)shift;
  }
  EntTables t;
  {
    std::lock_guard<std::mutex> lk(g_ent_mu);
    t = g_ent[h].t;
  }
  HIP_TRY(hipSetDevice(h->device));
  touch(h);
  if (t.cap_words < words) {
    uint32_t* fresh = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&fresh), words * sizeof(uint32_t)));
    if (t.d_tab) {  // kernels enqueued earlier may still read the old tables
      (void)hipStreamSynchronize(h->stream);
      (void)hipFree(t.d_tab);
    }
    t.d_tab = fresh;
    t.cap_words = words;
    std::lock_guard<std::mutex> lk(g_ent_mu);
    EntTables owned;  // owned from here on; no tables until the copy is done
    owned.d_tab = fresh;
    owned.cap_words = words;
    g_ent[h].t = owned;
  }
  HIP_TRY(hipMemcpyAsync(t.d_tab, host.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));  // `host` is free on return
  meta.d_tab = t.d_tab;
  meta.cap_words = t.cap_words;
  meta.K = (uint32_t)K;
  meta.ncum = (uint32_t)ncum;
  std::lock_guard<std::mutex> lk(g_ent_mu);
  g_ent[h].t = meta;
  return TIC_OK;
}
}  // namespace

extern "C" {

int tic_entropy_scratch_bytes(const int64_t* counts, int n_streams, uint32_t L, size_t* bytes) {
  if (!bytes) return fail(TIC_EINVAL, "null bytes");
  *bytes = 0;
  if (n_streams < 0) return fail(TIC_EINVAL, "n_streams %d is negative", n_streams);
  if (n_streams > 0 && !counts) return fail(TIC_EINVAL, "null per-stream array");
  if (!ent_L_ok(L)) return fail(TIC_EINVAL, "segment length %u must be a multiple of 4 in [4, 16384]", L);
  const char* why = "";
  const long long T = ent_segments(counts, n_streams, L, &why);
  if (T < 0) return fail(TIC_EINVAL, "%s", why);
  *bytes = ent_scratch(n_streams, T, L);
  return TIC_OK;
}

int tic_entropy_encode_device(tic_handle* h, const uint8_t* d_sym, const int64_t* sym_offsets, const int64_t* counts,
                              int n_streams, uint32_t L, void* d_scratch, size_t scratch_bytes, uint8_t* d_out,
                              size_t out_cap, uint64_t* d_sizes) {
  return ent_encode(h, d_sym, sym_offsets, counts, n_streams, L, d_scratch, scratch_bytes, d_out, out_cap, d_sizes,
                    1);
}

int tic_entropy_encode_ctx_device(tic_handle* h, const uint8_t* d_sym, const int64_t* sym_offsets,
                                  const int64_t* counts, int n_streams, uint32_t L, void* d_scratch,
                                  size_t scratch_bytes, uint8_t* d_out, size_t out_cap, uint64_t* d_sizes) {
  return ent_encode(h, d_sym, sym_offsets, counts, n_streams, L, d_scratch, scratch_bytes, d_out, out_cap, d_sizes,
                    2);
}

int tic_entropy_decode_device(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets,
                              const int64_t* blob_sizes, const int64_t* counts, int n_streams, uint8_t* d_sym,
                              const int64_t* sym_offsets, void* d_scratch, size_t scratch_bytes) {
  return ent_decode(h, d_blob, blob_offsets, blob_sizes, counts, n_streams, d_sym, sym_offsets, d_scratch,
                    scratch_bytes, 1);
}

int tic_entropy_decode_ctx_device(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets,
                                  const int64_t* blob_sizes, const int64_t* counts, int n_streams, uint8_t* d_sym,
                                  const int64_t* sym_offsets, void* d_scratch, size_t scratch_bytes) {
  return ent_decode(h, d_blob, blob_offsets, blob_sizes, counts, n_streams, d_sym, sym_offsets, d_scratch,
                    scratch_bytes, 2);
}

int tic_histogram_ctx_device(tic_handle* h, const uint8_t* d_sym, size_t n, int Q, int K, uint64_t* d_counts) {
  if (!h) return fail(TIC_EINVAL, "null handle");
  if (Q < 1 || Q > 256) return fail(TIC_EINVAL, "Q %d must be in [1, 256]", Q);
  if (K < 1 || K > 65536) return fail(TIC_EINVAL, "context count %d must be in [1, 65536]", K);
  if (n == 0) return TIC_OK;
  if (!d_sym || !d_counts) return fail(TIC_EINVAL, "null argument");
  if (((uintptr_t)d_counts & 7) != 0) return fail(TIC_EINVAL, "d_counts must be 8-byte aligned");
  HIP_TRY(hipSetDevice(h->device));
  touch(h);
  // rows of K symbols over blockIdx.y: enough lanes to fill the device, at most one per row
  const size_t rows = (n + (size_t)K - 1) / (size_t)K;
  const unsigned gx = ((unsigned)K + 255) / 256;
  const size_t want = std::max<size_t>(1, (size_t)h->num_cus * 8 / gx);
  const unsigned gy = (unsigned)std::min<size_t>(std::min(rows, want), 65535);
  hipLaunchKernelGGL(tic::ent_histogram_ctx_kernel, dim3(gx, gy), dim3(256), 0, h->stream, d_sym, n, Q, (uint32_t)K,
                     reinterpret_cast<unsigned long long*>(d_counts));
  return check_launch();
}

int tic_entropy_encode_nbr_device(tic_handle* h, const uint8_t* d_sym, const int64_t* sym_offsets,
                                  const int64_t* counts, int n_streams, uint32_t L, void* d_scratch,
                                  size_t scratch_bytes, uint8_t* d_out, size_t out_cap, uint64_t* d_sizes) {
  return ent_encode(h, d_sym, sym_offsets, counts, n_streams, L, d_scratch, scratch_bytes, d_out, out_cap, d_sizes,
                    3);
}

int tic_entropy_decode_nbr_device(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets,
                                  const int64_t* blob_sizes, const int64_t* counts, int n_streams, uint8_t* d_sym,
                                  const int64_t* sym_offsets, void* d_scratch, size_t scratch_bytes) {
  return ent_decode(h, d_blob, blob_offsets, blob_sizes, counts, n_streams, d_sym, sym_offsets, d_scratch,
                    scratch_bytes, 3);
}

int tic_entropy_ranges_scratch_bytes(const int64_t* firsts, const int64_t* counts, int n_ranges, uint32_t L,
                                     size_t* bytes) {
  if (!bytes) return fail(TIC_EINVAL, "null bytes");
  *bytes = 0;
  if (n_ranges < 0) return fail(TIC_EINVAL, "n_ranges %d is negative", n_ranges);
  if (n_ranges > 0 && (!firsts || !counts)) return fail(TIC_EINVAL, "null per-range array");
  if (!ent_L_ok(L)) return fail(TIC_EINVAL, "segment length %u must be a multiple of 4 in [4, 16384]", L);
  long long T = 0;
  for (int i = 0; i < n_ranges; ++i) {
    if (firsts[i] < 0 || counts[i] <= 0 || counts[i] > (1ll << 40))
      return fail(TIC_EINVAL, "range %d: first %lld, count %lld", i, (long long)firsts[i], (long long)counts[i]);
    T += ent_range_segments(counts[i], L);
    if (T > INT_MAX) return fail(TIC_EINVAL, "more than 2^31 - 1 segments");
  }
  *bytes = ent_fixed(n_ranges) + (size_t)n_ranges * sizeof(tic::EntRng) + (size_t)T * 8;
  return TIC_OK;
}

int tic_entropy_decode_ranges_device(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets,
                                     const int64_t* blob_sizes, const int64_t* stream_counts, const int64_t* firsts,
                                     const int64_t* counts, int n_ranges, uint8_t* d_sym, const int64_t* sym_offsets,
                                     void* d_scratch, size_t scratch_bytes) {
  return ent_decode_ranges(h, d_blob, blob_offsets, blob_sizes, stream_counts, firsts, counts, n_ranges, d_sym,
                           sym_offsets, d_scratch, scratch_bytes, 1);
}

int tic_entropy_decode_ranges_ctx_device(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets,
                                         const int64_t* blob_sizes, const int64_t* stream_counts,
                                         const int64_t* firsts, const int64_t* counts, int n_ranges, uint8_t* d_sym,
                                         const int64_t* sym_offsets, void* d_scratch, size_t scratch_bytes) {
  return ent_decode_ranges(h, d_blob, blob_offsets, blob_sizes, stream_counts, firsts, counts, n_ranges, d_sym,
                           sym_offsets, d_scratch, scratch_bytes, 2);
}

int tic_entropy_decode_ranges_nbr_device(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets,
                                         const int64_t* blob_sizes, const int64_t* stream_counts,
                                         const int64_t* firsts, const int64_t* counts, int n_ranges, uint8_t* d_sym,
                                         const int64_t* sym_offsets, void* d_scratch, size_t scratch_bytes) {
  return ent_decode_ranges(h, d_blob, blob_offsets, blob_sizes, stream_counts, firsts, counts, n_ranges, d_sym,
                           sym_offsets, d_scratch, scratch_bytes, 3);
}

int tic_histogram_nbr_device(tic_handle* h, const uint8_t* d_sym, const int64_t* sym_offsets, const int64_t* counts,
                             int n_streams, int Q, uint32_t L, uint64_t* d_counts) {
  if (!h) return fail(TIC_EINVAL, "null handle");
  if (Q < 1 || Q > 256) return fail(TIC_EINVAL, "Q %d must be in [1, 256]", Q);
  if (n_streams < 0) return fail(TIC_EINVAL, "n_streams %d is negative", n_streams);
  if (!ent_L_ok(L)) return fail(TIC_EINVAL, "segment length %u must be a multiple of 4 in [4, 16384]", L);
  EntTables tb;
  int rc = ent_tables(h, &tb, true);
  if (rc) return rc;
  if (n_streams == 0) return TIC_OK;
  if (!d_sym || !d_counts) return fail(TIC_EINVAL, "null device pointer");
  if (!sym_offsets || !counts) return fail(TIC_EINVAL, "null per-stream array");
  if (((uintptr_t)d_counts & 7) != 0) return fail(TIC_EINVAL, "d_counts must be 8-byte aligned");
  const char* why = "";
  if (ent_segments(counts, n_streams, L, &why) < 0) return fail(TIC_EINVAL, "%s", why);
  for (int i = 0; i < n_streams; ++i)
    if (sym_offsets[i] < 0) return fail(TIC_EINVAL, "stream %d: negative offset %lld", i, (long long)sym_offsets[i]);
  HIP_TRY(hipSetDevice(h->device));
  const tic::EntNbr q = ent_nbr(tb);
  for (int f = 0; f < n_streams; f += tic::kEntStreams) {
    tic::EntChunk t;
    memset(&t, 0, sizeof(t));
    t.n = std::min(tic::kEntStreams, n_streams - f);
    t.first = f;
    long long most = 0;
    for (int k = 0; k < t.n; ++k) {
      t.in_off[k] = sym_offsets[f + k];
      t.count[k] = counts[f + k];
      most = std::max(most, (long long)counts[f + k]);
    }
    // pieces of 64 symbols, 256 to a workgroup
    const unsigned gx = (unsigned)std::min<long long>((most / 64 + 256) / 256, (long long)h->num_cus * 8);
    touch(h);
    hipLaunchKernelGGL(tic::ent_histogram_nbr_kernel, dim3(gx, (unsigned)t.n), dim3(256), 0, h->stream, t, q, d_sym, Q,
                       L, reinterpret_cast<unsigned long long*>(d_counts));
    if ((rc = check_launch())) return rc;
  }
  return TIC_OK;
}

}  // extern "C"

namespace {

int ent_encode(tic_handle* h, const uint8_t* d_sym, const int64_t* sym_offsets, const int64_t* counts, int n_streams,
               uint32_t L, void* d_scratch, size_t scratch_bytes, uint8_t* d_out, size_t out_cap, uint64_t* d_sizes,
               int ver) {
  const bool ctx = ver >= 2, nbr = ver == 3;  // ctx: tables in the handle's buffer
  const size_t hdr = nbr ? 36 : ctx ? 28 : 20;
  if (!h) return fail(TIC_EINVAL, "null handle");
  if (n_streams < 0) return fail(TIC_EINVAL, "n_streams %d is negative", n_streams);
  if (n_streams == 0) return TIC_OK;
  if (!d_sym || !d_scratch || !d_out || !d_sizes) return fail(TIC_EINVAL, "null device pointer");
  if (!sym_offsets || !counts) return fail(TIC_EINVAL, "null per-stream array");
  if (!ent_L_ok(L)) return fail(TIC_EINVAL, "segment length %u must be a multiple of 4 in [4, 16384]", L);
  const char* why = "";
  const long long T = ent_segments(counts, n_streams, L, &why);
  if (T < 0) return fail(TIC_EINVAL, "%s", why);
  size_t bound = 0;
  for (int i = 0; i < n_streams; ++i) {
    if (sym_offsets[i] < 0) return fail(TIC_EINVAL, "stream %d: negative offset %lld", i, (long long)sym_offsets[i]);
    const size_t S = ((size_t)counts[i] + L - 1) / L;
    bound += hdr + 2 * S + 3 * (size_t)counts[i] + 4 * S;
  }
  tic::EntModel m;
  EntTables tb;
  int rc = ctx ? ent_tables(h, &tb, nbr) : ent_model(h, &m);
  if (rc) return rc;
  if (((uintptr_t)d_scratch & 15) != 0 || ((uintptr_t)d_sizes & 7) != 0)
    return fail(TIC_EINVAL, "d_scratch must be 16-byte and d_sizes 8-byte aligned");
  const size_t need = ent_scratch(n_streams, T, L);
  if (scratch_bytes < need)
    return fail(TIC_EINVAL, "scratch of %zu bytes is too small (tic_entropy_scratch_bytes: %zu)", scratch_bytes, need);
  if (out_cap < bound)
    return fail(TIC_EINVAL, "out_cap %zu is below the sum of tic_rcseg_bound%s (%zu)", out_cap, nbr ? "_nbr" : ctx ? "_ctx" : "",
                bound);
  const size_t tab_bytes = ctx ? (size_t)tb.K * tb.ncum * sizeof(uint32_t) : 0;
  const bool in_lds = tab_bytes <= kEntLdsTables;

  HIP_TRY(hipSetDevice(h->device));
  if (ctx && in_lds && tab_bytes > 48 * 1024)
    HIP_TRY(hipFuncSetAttribute(nbr ? reinterpret_cast<const void*>(tic::ent_encode_nbr_kernel<1>)
                                    : reinterpret_cast<const void*>(tic::ent_encode_ctx_kernel<1>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)tab_bytes));
  const tic::EntNbr q = nbr ? ent_nbr(tb) : tic::EntNbr{};
  const uint32_t g0 = nbr ? tb.eh | tb.ew << 16 : 0, g1 = nbr ? tb.C | tb.neighbours << 16 : 0;
  const EntScratch s = ent_carve(d_scratch, n_streams, T);
  long long segs = 0;
  for (int f = 0; f < n_streams; f += tic::kEntStreams) {
    tic::EntChunk t;
    memset(&t, 0, sizeof(t));
    t.n = std::min(tic::kEntStreams, n_streams - f);
    t.first = f;
    t.last = f + t.n == n_streams;
    for (int k = 0; k < t.n; ++k) {
      t.in_off[k] = sym_offsets[f + k];
      t.count[k] = counts[f + k];
      t.seg_base[k] = segs;
      segs += (counts[f + k] + L - 1) / L;
    }
    t.seg_base[t.n] = segs;
    touch(h);
    hipLaunchKernelGGL(tic::ent_put_kernel, dim3(1), dim3(64), 0, h->stream, t, L, s.rec, s.seg_base);
    if ((rc = check_launch())) return rc;
  }
  const unsigned wgs = (unsigned)((T + 63) / 64);
  const tic::EntRec* rec = s.rec;
  const unsigned long long* seg_base = s.seg_base;
  if (!ctx)
    hipLaunchKernelGGL(tic::ent_encode_kernel, dim3(wgs), dim3(64), 0, h->stream, m, d_sym, rec, seg_base, n_streams,
                       L, s.slots, s.seg_len);
  else if (nbr && in_lds)
    hipLaunchKernelGGL(tic::ent_encode_nbr_kernel<1>, dim3(wgs), dim3(64), tab_bytes, h->stream,
                       (const uint32_t*)tb.d_tab, q, d_sym, rec, seg_base, n_streams, L, s.slots, s.seg_len);
  else if (nbr)
    hipLaunchKernelGGL(tic::ent_encode_nbr_kernel<0>, dim3(wgs), dim3(64), 0, h->stream, (const uint32_t*)tb.d_tab, q,
                       d_sym, rec, seg_base, n_streams, L, s.slots, s.seg_len);
  else if (in_lds)
    hipLaunchKernelGGL(tic::ent_encode_ctx_kernel<1>, dim3(wgs), dim3(64), tab_bytes, h->stream,
                       (const uint32_t*)tb.d_tab, tb.K, tb.ncum, d_sym, rec, seg_base, n_streams, L, s.slots,
                       s.seg_len);
  else
    hipLaunchKernelGGL(tic::ent_encode_ctx_kernel<0>, dim3(wgs), dim3(64), 0, h->stream, (const uint32_t*)tb.d_tab,
                       tb.K, tb.ncum, d_sym, rec, seg_base, n_streams, L, s.slots, s.seg_len);
  if ((rc = check_launch())) return rc;
  unsigned long long* sizes = reinterpret_cast<unsigned long long*>(d_sizes);
  const uint32_t* seg_len = s.seg_len;
  if (nbr)
    hipLaunchKernelGGL(tic::ent_seg_scan_kernel<36>, dim3((unsigned)n_streams), dim3(256), 0, h->stream, rec, seg_base,
                       seg_len, s.seg_off, sizes);
  else if (ctx)
    hipLaunchKernelGGL(tic::ent_seg_scan_kernel<28>, dim3((unsigned)n_streams), dim3(256), 0, h->stream, rec, seg_base,
                       seg_len, s.seg_off, sizes);
  else
    hipLaunchKernelGGL(tic::ent_seg_scan_kernel<20>, dim3((unsigned)n_streams), dim3(256), 0, h->stream, rec, seg_base,
                       seg_len, s.seg_off, sizes);
  if ((rc = check_launch())) return rc;
  hipLaunchKernelGGL(tic::ent_stream_scan_kernel, dim3(1), dim3(256), 0, h->stream, (const unsigned long long*)sizes,
                     n_streams, s.aux);
  if ((rc = check_launch())) return rc;
  const uint8_t* slots = s.slots;
  const unsigned long long *seg_off = s.seg_off, *csizes = sizes, *out_off = s.aux;
  if (nbr)
    hipLaunchKernelGGL(tic::ent_gather_kernel<36>, dim3((unsigned)T), dim3(256), 0, h->stream, rec, seg_base,
                       n_streams, L, slots, seg_len, seg_off, csizes, out_off, tb.K0, tb.crc, g0, g1, d_out);
  else if (ctx)
    hipLaunchKernelGGL(tic::ent_gather_kernel<28>, dim3((unsigned)T), dim3(256), 0, h->stream, rec, seg_base,
                       n_streams, L, slots, seg_len, seg_off, csizes, out_off, tb.K, tb.crc, 0u, 0u, d_out);
  else
    hipLaunchKernelGGL(tic::ent_gather_kernel<20>, dim3((unsigned)T), dim3(256), 0, h->stream, rec, seg_base,
                       n_streams, L, slots, seg_len, seg_off, csizes, out_off, 0u, 0u, 0u, 0u, d_out);
  return check_launch();
}

// RNG = 0: whole containers (firsts, rcounts unused); 1: one symbol range per record.
template <int RNG>
int ent_decode_t(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets, const int64_t* blob_sizes,
                 const int64_t* counts, const int64_t* firsts, const int64_t* rcounts, int n_streams, uint8_t* d_sym,
                 const int64_t* sym_offsets, void* d_scratch, size_t scratch_bytes, int ver) {
  const bool ctx = ver >= 2, nbr = ver == 3;
  if (!h) return fail(TIC_EINVAL, "null handle");
  if (n_streams < 0) return fail(TIC_EINVAL, "n_streams %d is negative", n_streams);
  if (n_streams == 0) return TIC_OK;
  if (!d_blob || !d_scratch || !d_sym) return fail(TIC_EINVAL, "null device pointer");
  if (!blob_offsets || !blob_sizes || !counts || !sym_offsets) return fail(TIC_EINVAL, "null per-stream array");
  if (RNG && (!firsts || !rcounts)) return fail(TIC_EINVAL, "null per-range array");
  const char* why = "";
  long long Tmin = ent_segments(counts, n_streams, tic::kEntMaxL, &why);
  if (Tmin < 0) return fail(TIC_EINVAL, "%s", why);
  if (RNG) {
    Tmin = n_streams;  // a range touches at least one segment
    for (int i = 0; i < n_streams; ++i)
      if (firsts[i] < 0 || rcounts[i] <= 0 || firsts[i] >= counts[i] || rcounts[i] > counts[i] - firsts[i])
        return fail(TIC_EINVAL, "range %d: [%lld, %lld + %lld) is empty or not inside the stream's %lld symbols", i,
                    (long long)firsts[i], (long long)firsts[i], (long long)rcounts[i], (long long)counts[i]);
  }
  for (int i = 0; i < n_streams; ++i)
    if (blob_offsets[i] < 0 || blob_sizes[i] < 0 || sym_offsets[i] < 0)
      return fail(TIC_EINVAL, "stream %d: negative offset or size", i);
  tic::EntModel m;
  EntTables tb;
  int rc = ctx ? ent_tables(h, &tb, nbr) : ent_model(h, &m);
  if (rc) return rc;
  if (((uintptr_t)d_scratch & 15) != 0) return fail(TIC_EINVAL, "d_scratch must be 16-byte aligned");
  // RNG: the ranges lie between the records and the per-segment offsets
  const size_t fixed = ent_fixed(n_streams) + (RNG ? (size_t)n_streams * sizeof(tic::EntRng) : 0);
  if (scratch_bytes < fixed + (size_t)Tmin * 8)
    return fail(TIC_EINVAL, "scratch of %zu bytes is too small (tic_entropy_%sscratch_bytes)", scratch_bytes,
                RNG ? "ranges_" : "");
  // segments the scratch has room for: the containers' own L decides how many there are
  const unsigned long long cap = std::min<unsigned long long>((scratch_bytes - fixed) / 8, INT_MAX);

  const uint32_t total = ctx ? 0 : m.cum[m.nsym];
  const int lut = !ctx && total <= tic::kEntLutMax;
  const size_t tab_bytes = ctx ? (size_t)tb.K * tb.ncum * sizeof(uint32_t) : 0;
  const bool in_lds = tab_bytes <= kEntLdsTables;
  const tic::EntNbr q = nbr ? ent_nbr(tb) : tic::EntNbr{};
  const uint32_t g0 = nbr ? tb.eh | tb.ew << 16 : 0, g1 = nbr ? tb.C | tb.neighbours << 16 : 0;
  // version 3: a lane's ring of class bits, whole words, for each of a workgroup's 64 lanes
  size_t ring_bytes = nbr ? ((size_t)q.ring + 31) / 32 * 4 * 64 : 0;
  const bool ring = ring_bytes <= kEntLdsRings;
  // RNG && !ring: 32 working lanes a workgroup, their rings in LDS all the same
  const unsigned lanes = RNG && !ring ? 32 : 64;
  if (RNG && !ring) ring_bytes /= 2;
  const size_t lds = ctx ? (in_lds ? tab_bytes : 0) + (ring || RNG ? ring_bytes : 0)
                         : 260 * sizeof(uint32_t) + (lut ? ((size_t)total + 3) / 4 * 4 : 0);
  const void* dec_nbr = in_lds ? (ring ? reinterpret_cast<const void*>(tic::ent_decode_nbr_kernel<1, 1, RNG>)
                                       : reinterpret_cast<const void*>(tic::ent_decode_nbr_kernel<1, 0, RNG>))
                               : (ring ? reinterpret_cast<const void*>(tic::ent_decode_nbr_kernel<0, 1, RNG>)
                                       : reinterpret_cast<const void*>(tic::ent_decode_nbr_kernel<0, 0, RNG>));
  HIP_TRY(hipSetDevice(h->device));
  if (lds > 48 * 1024)
    HIP_TRY(hipFuncSetAttribute(nbr   ? dec_nbr
                                : ctx ? reinterpret_cast<const void*>(tic::ent_decode_ctx_kernel<1, RNG>)
                                      : reinterpret_cast<const void*>(tic::ent_decode_kernel<RNG>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  EntScratch s = ent_carve(d_scratch, n_streams, 0);
  tic::EntRng* rng = RNG ? reinterpret_cast<tic::EntRng*>(s.seg_off) : nullptr;
  s.seg_off = reinterpret_cast<unsigned long long*>(static_cast<uint8_t*>(d_scratch) + fixed);
  for (int f = 0; f < n_streams; f += tic::kEntStreams) {
    tic::EntChunk t;
    memset(&t, 0, sizeof(t));
    t.n = std::min(tic::kEntStreams, n_streams - f);
    t.first = f;
    for (int k = 0; k < t.n; ++k) {
      t.in_off[k] = blob_offsets[f + k];
      t.in_size[k] = blob_sizes[f + k];
      t.count[k] = counts[f + k];
      t.out_off[k] = sym_offsets[f + k];
    }
    tic::EntRngChunk<RNG> rg;
    if constexpr (RNG != 0) {
      memset(&rg, 0, sizeof(rg));
      for (int k = 0; k < t.n; ++k) rg.first[k] = firsts[f + k], rg.count[k] = rcounts[f + k];
    }
    touch(h);
    if (nbr)
      hipLaunchKernelGGL((tic::ent_dec_header_kernel<36, RNG>), dim3(1), dim3(64), 0, h->stream,
                         t, d_blob, tb.K0, tb.crc, g0,
                         g1, s.rec, s.aux, rg, rng);
    else if (ctx)
      hipLaunchKernelGGL((tic::ent_dec_header_kernel<28, RNG>), dim3(1), dim3(64), 0, h->stream,
                         t, d_blob, tb.K, tb.crc, 0u,
                         0u, s.rec, s.aux, rg, rng);
    else
      hipLaunchKernelGGL((tic::ent_dec_header_kernel<20, RNG>), dim3(1), dim3(64), 0, h->stream,
                         t, d_blob, 0u, 0u, 0u, 0u,
                         s.rec, s.aux, rg, rng);
    if ((rc = check_launch())) return rc;
  }
  hipLaunchKernelGGL(tic::ent_stream_scan_kernel, dim3(1), dim3(256), 0, h->stream, (const unsigned long long*)s.aux,
                     n_streams, s.seg_base);
  if ((rc = check_launch())) return rc;
  const unsigned long long* seg_base = s.seg_base;
  const tic::EntRng* crng = rng;
  if (nbr)
    hipLaunchKernelGGL((tic::ent_dec_scan_kernel<36, RNG>), dim3((unsigned)n_streams), dim3(256), 0, h->stream,
                       d_blob, s.rec,
                       seg_base, cap, s.seg_off, d_sym, crng);
  else if (ctx)
    hipLaunchKernelGGL((tic::ent_dec_scan_kernel<28, RNG>), dim3((unsigned)n_streams), dim3(256), 0, h->stream,
                       d_blob, s.rec,
                       seg_base, cap, s.seg_off, d_sym, crng);
  else
    hipLaunchKernelGGL((tic::ent_dec_scan_kernel<20, RNG>), dim3((unsigned)n_streams), dim3(256), 0, h->stream,
                       d_blob, s.rec,
                       seg_base, cap, s.seg_off, d_sym, crng);
  if ((rc = check_launch())) return rc;
  const unsigned wgs = (unsigned)std::min<unsigned long long>((cap + lanes - 1) / lanes, 1u << 16);
  const tic::EntRec* rec = s.rec;
  const unsigned long long* seg_off = s.seg_off;
  if (!ctx)
    hipLaunchKernelGGL(tic::ent_decode_kernel<RNG>, dim3(wgs), dim3(64), lds, h->stream, m, lut, d_blob, rec, seg_base,
                       n_streams, seg_off, d_sym, crng);
  else if (nbr && in_lds && ring)
    hipLaunchKernelGGL((tic::ent_decode_nbr_kernel<1, 1, RNG>), dim3(wgs), dim3(64), lds, h->stream,
                       (const uint32_t*)tb.d_tab, q, d_blob, rec, seg_base, n_streams, seg_off, d_sym, crng);
  else if (nbr && in_lds)
    hipLaunchKernelGGL((tic::ent_decode_nbr_kernel<1, 0, RNG>), dim3(wgs), dim3(64), lds, h->stream,
                       (const uint32_t*)tb.d_tab, q, d_blob, rec, seg_base, n_streams, seg_off, d_sym, crng);
  else if (nbr && ring)
    hipLaunchKernelGGL((tic::ent_decode_nbr_kernel<0, 1, RNG>), dim3(wgs), dim3(64), lds, h->stream,
                       (const uint32_t*)tb.d_tab, q, d_blob, rec, seg_base, n_streams, seg_off, d_sym, crng);
  else if (nbr)
    hipLaunchKernelGGL((tic::ent_decode_nbr_kernel<0, 0, RNG>), dim3(wgs), dim3(64), lds, h->stream,
                       (const uint32_t*)tb.d_tab, q, d_blob, rec, seg_base, n_streams, seg_off, d_sym, crng);
  else if (in_lds)
    hipLaunchKernelGGL((tic::ent_decode_ctx_kernel<1, RNG>), dim3(wgs), dim3(64), lds, h->stream,
                       (const uint32_t*)tb.d_tab,
                       tb.K, tb.ncum, d_blob, rec, seg_base, n_streams, seg_off, d_sym, crng);
  else
    hipLaunchKernelGGL((tic::ent_decode_ctx_kernel<0, RNG>), dim3(wgs), dim3(64), 0, h->stream,
                       (const uint32_t*)tb.d_tab,
                       tb.K, tb.ncum, d_blob, rec, seg_base, n_streams, seg_off, d_sym, crng);
  return check_launch();
}


int ent_decode(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets, const int64_t* blob_sizes,
               const int64_t* counts, int n_streams, uint8_t* d_sym, const int64_t* sym_offsets, void* d_scratch,
               size_t scratch_bytes, int ver) {
  return ent_decode_t<0>(h, d_blob, blob_offsets, blob_sizes, counts, nullptr, nullptr, n_streams, d_sym, sym_offsets,
                         d_scratch, scratch_bytes, ver);
}

int ent_decode_ranges(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets, const int64_t* blob_sizes,
                      const int64_t* counts, const int64_t* firsts, const int64_t* rcounts, int n_ranges,
                      uint8_t* d_sym, const int64_t* sym_offsets, void* d_scratch, size_t scratch_bytes, int ver) {
  return ent_decode_t<1>(h, d_blob, blob_offsets, blob_sizes, counts, firsts, rcounts, n_ranges, d_sym, sym_offsets,
                         d_scratch, scratch_bytes, ver);
}

}  // namespace
