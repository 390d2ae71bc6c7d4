// What does v_mul_lo_u32 cost on gfx950 next to v_mul_u32_u24 and v_add_u32?  (The field kernel's gather block forms
// cy * pa and cz * pb with twelve v_mul_lo_u32 per tile; where mask, stride and stride^2 of a level fit 24 bits the
// 24-bit multiply gives the same row.)  Four independent chains per lane, 256 instructions per loop trip, every SIMD
// of the chip busy with two waves: the time per instruction relative to v_add_u32 is the issue price relative to a
// plain VALU instruction.
//   hipcc --offload-arch=gfx950 -O3 tools/micro/mul24_bench.hip -o tools/micro/mul24_bench && tools/micro/mul24_bench
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>

#define CHAIN4(op)                                                                                      \
  asm volatile(".rept 64\n" op " %0, %0, %4\n" op " %1, %1, %4\n" op " %2, %2, %4\n" op " %3, %3, %4\n" \
               ".endr"                                                                                  \
               : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3)                                                 \
               : "v"(b))

template <int OP>
__global__ void __launch_bounds__(256) k(uint32_t* out, uint32_t a, uint32_t b, int trips) {
  uint32_t x0 = threadIdx.x + a, x1 = x0 ^ b, x2 = x0 + b, x3 = x1 + 7u;
  for (int i = 0; i < trips; ++i) {
    if (OP == 0) CHAIN4("v_add_u32");
    if (OP == 1) CHAIN4("v_mul_u32_u24");
    if (OP == 2) CHAIN4("v_mul_lo_u32");
  }
  out[blockIdx.x * 256 + threadIdx.x] = x0 ^ x1 ^ x2 ^ x3;
}

template <int OP>
static float run(uint32_t* out, int blocks, int trips) {
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  k<OP><<<blocks, 256>>>(out, 3u, 2654435761u, 8);      // warm-up
  float best = 1e30f;
  for (int r = 0; r < 5; ++r) {
    (void)hipEventRecord(e0);
    k<OP><<<blocks, 256>>>(out, 3u, 2654435761u, trips);
    (void)hipEventRecord(e1);
    if (hipEventSynchronize(e1) != hipSuccess) return -1.0f;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    best = ms < best ? ms : best;
  }
  return best;
}

int main() {
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, 0) != hipSuccess) { printf("no device\n"); return 1; }
  const int blocks = p.multiProcessorCount * 2, trips = 4096;      // 2 workgroups of 4 waves per CU: 2 waves per SIMD
  uint32_t* out;
  if (hipMalloc(&out, (size_t)blocks * 256 * 4) != hipSuccess) return 1;
  const float add = run<0>(out, blocks, trips), m24 = run<1>(out, blocks, trips), mlo = run<2>(out, blocks, trips);
  if (add < 0 || m24 < 0 || mlo < 0) { printf("launch failed\n"); return 1; }
  const double per_simd = 2.0 * trips * 256.0;                     // instructions issued per SIMD
  printf("%s, %d CUs, %d instructions per SIMD per launch (best of 5)\n", p.gcnArchName, p.multiProcessorCount, (int)per_simd);
  printf("v_add_u32      %8.3f ms  %6.3f ns/instr  1.00x\n", add, add * 1e6 / per_simd);
  printf("v_mul_u32_u24  %8.3f ms  %6.3f ns/instr  %.2fx\n", m24, m24 * 1e6 / per_simd, m24 / add);
  printf("v_mul_lo_u32   %8.3f ms  %6.3f ns/instr  %.2fx\n", mlo, mlo * 1e6 / per_simd, mlo / add);
  (void)hipFree(out);
  return 0;
}
