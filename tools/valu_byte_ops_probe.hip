// valu_byte_ops_probe.hip — issue rate of the byte instructions blur_match_tiled_kernel is made of, on the device it runs
// on: v_dot4_u32_u8, v_sad_u8 and v_alignbyte_b32, next to v_add_u32 and v_mad_u32_u24 as yardsticks.  Every thread keeps
// CHAINS independent accumulators in registers and applies the instruction ITER times to each, so the dependent-issue
// latency is covered and nothing touches memory until the end.  Prints one line per instruction: lane-operations per
// second, wave-instructions per CU and clock (from the device's reported clock), and byte-MACs per second where that
// means something.  profiles/r26_match.md quotes it.
//
//   hipcc --offload-arch=gfx950 -O3 -o valu_byte_ops_probe tools/valu_byte_ops_probe.hip && ./valu_byte_ops_probe
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>

constexpr int CHAINS = 8, ITER = 4096, THREADS = 256;

enum Op { DOT4, SAD, ALIGN, ADD, MAD24 };

template <int OP>
__global__ __launch_bounds__(THREADS) void probe_kernel(uint32_t *out, uint32_t a0, uint32_t b0)
{
    uint32_t acc[CHAINS], a = a0 + threadIdx.x, b = b0 ^ blockIdx.x;
#pragma unroll
    for (int c = 0; c < CHAINS; c++) acc[c] = c;
    for (int i = 0; i < ITER; i++) {
#pragma unroll
        for (int c = 0; c < CHAINS; c++) {
            if (OP == DOT4) acc[c] = __builtin_amdgcn_udot4(a, b, acc[c], false);
            if (OP == SAD) acc[c] = __builtin_amdgcn_sad_u8(a, b, acc[c]);
            if (OP == ALIGN) acc[c] = __builtin_amdgcn_alignbyte(acc[c], a, b);
            if (OP == ADD) asm volatile("v_add_u32 %0, %1, %0" : "+v"(acc[c]) : "v"(a));
            if (OP == MAD24) acc[c] = __umul24(a, b) + acc[c];
        }
        if (OP != ADD) asm volatile("" : "+v"(a), "+v"(b));             // the operands stay run-time values: nothing is folded
    }
    uint32_t s = 0;
#pragma unroll
    for (int c = 0; c < CHAINS; c++) s += acc[c];
    if (s == 0x12345678u) out[0] = s;                                   // keeps the chains alive; practically never taken
}

template <int OP>
static void run(const char *name, int macs_per_op, uint32_t *d_out, int cus, double clock_hz)
{
    const int blocks = cus * 16;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    double best = 1e30;
    for (int rep = 0; rep < 6; rep++) {                                 // the first launches ramp the clock
        (void)hipEventRecord(e0, nullptr);
        hipLaunchKernelGGL(probe_kernel<OP>, dim3(blocks), dim3(THREADS), 0, nullptr, d_out, 0x01020304u + rep, 0x05060703u);
        (void)hipEventRecord(e1, nullptr);
        if (hipEventSynchronize(e1) != hipSuccess) { printf("%s: launch failed\n", name); return; }
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        if (rep >= 2 && ms < best) best = ms;
    }
    const double lane_ops = (double)blocks * THREADS * CHAINS * ITER, s = best * 1e-3;
    const double wave_instr_per_cu_clk = lane_ops / 64.0 / s / cus / clock_hz;
    printf("%-16s %8.3f ms  %9.2f G lane-ops/s  %6.3f wave-instr/CU/clk", name, best, lane_ops / s * 1e-9, wave_instr_per_cu_clk);
    if (macs_per_op) printf("  %8.2f T byte-MAC/s", lane_ops * macs_per_op / s * 1e-12);
    printf("\n");
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
}

int main()
{
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { printf("no HIP device\n"); return 1; }
    const int cus = prop.multiProcessorCount;
    const double clock_hz = prop.clockRate * 1e3;
    printf("%s: %d CUs, %.0f MHz reported\n", prop.name, cus, clock_hz * 1e-6);
    uint32_t *d_out = nullptr;
    if (hipMalloc(&d_out, 64) != hipSuccess) return 1;
    run<DOT4>("v_dot4_u32_u8", 4, d_out, cus, clock_hz);
    run<SAD>("v_sad_u8", 4, d_out, cus, clock_hz);
    run<ALIGN>("v_alignbyte_b32", 0, d_out, cus, clock_hz);
    run<ADD>("v_add_u32", 0, d_out, cus, clock_hz);
    run<MAD24>("v_mad_u32_u24", 0, d_out, cus, clock_hz);
    (void)hipFree(d_out);
    return 0;
}
