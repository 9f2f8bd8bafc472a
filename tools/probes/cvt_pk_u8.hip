// Micro-probe: does v_cvt_pk_u8_f32 round to nearest even on its own?  The last layer's store
// (convT_rgb_valu.h rgb_out_pack4) feeds it clipped values of [0, 255] without a v_rndne_f32
// before it, which is right only if every such float converts as (uint8)rintf(x) does.  Checks
// every float bit pattern from +0 to 255.0, in every byte position; prints the number of
// mismatches and the first one.  Exit status 0: none.
//   hipcc --offload-arch=gfx950 -O3 tools/probes/cvt_pk_u8.hip -o tools/probes/cvt_pk_u8 && tools/probes/cvt_pk_u8
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>

__global__ void __launch_bounds__(256) probe(unsigned last, unsigned long long* bad, unsigned* first) {
  const unsigned stride = gridDim.x * blockDim.x;
  for (unsigned long long b = blockIdx.x * blockDim.x + threadIdx.x; b <= last; b += stride) {
    const float x = __uint_as_float((unsigned)b);
    const unsigned want = (unsigned)rintf(x);
    bool ok = true;
    ok &= __builtin_amdgcn_cvt_pk_u8_f32(x, 0, 0xA5A5A5A5u) == ((0xA5A5A5A5u & ~0xffu) | want);
    ok &= __builtin_amdgcn_cvt_pk_u8_f32(x, 1, 0xA5A5A5A5u) == ((0xA5A5A5A5u & ~0xff00u) | (want << 8));
    ok &= __builtin_amdgcn_cvt_pk_u8_f32(x, 2, 0xA5A5A5A5u) == ((0xA5A5A5A5u & ~0xff0000u) | (want << 16));
    ok &= __builtin_amdgcn_cvt_pk_u8_f32(x, 3, 0xA5A5A5A5u) == ((0xA5A5A5A5u & ~0xff000000u) | (want << 24));
    if (!ok) {
      atomicAdd(bad, 1ull);
      atomicMin(first, (unsigned)b);
    }
  }
}

int main() {
  unsigned long long* bad;
  unsigned* first;
  if (hipMalloc((void**)&bad, 8) != hipSuccess || hipMalloc((void**)&first, 4) != hipSuccess) return 2;
  const unsigned long long zero = 0;
  const unsigned none = 0xffffffffu;
  (void)hipMemcpy(bad, &zero, 8, hipMemcpyHostToDevice);
  (void)hipMemcpy(first, &none, 4, hipMemcpyHostToDevice);
  const float top = 255.0f;
  unsigned last;
  __builtin_memcpy(&last, &top, 4);
  hipLaunchKernelGGL(probe, dim3(4096), dim3(256), 0, 0, last, bad, first);
  unsigned long long nbad = ~0ull;
  unsigned f = 0;
  if (hipDeviceSynchronize() != hipSuccess) return 2;
  (void)hipMemcpy(&nbad, bad, 8, hipMemcpyDeviceToHost);
  (void)hipMemcpy(&f, first, 4, hipMemcpyDeviceToHost);
  float fx;
  __builtin_memcpy(&fx, &f, 4);
  printf("v_cvt_pk_u8_f32 vs (uint8)rintf over %u floats of [0, 255]: %llu mismatches", last + 1, nbad);
  if (nbad) printf(" (first at %.9g, bits 0x%08x)", fx, f);
  printf("\n");
  return nbad ? 1 : 0;
}
