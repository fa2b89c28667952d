// Issue rate of the integer vector instructions the ORB kernels are made of, on gfx950, 8 waves per SIMD (everything resident at once):
// hipcc -O3 --offload-arch=gfx950 tools/probes/valu_rate.hip -o /tmp/valu_rate && /tmp/valu_rate
#include <hip/hip_runtime.h>
#include <cstdio>
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
typedef short ss2 __attribute__((ext_vector_type(2)));
template <int OP>
__global__ __launch_bounds__(512) void k(unsigned* out, int iters, unsigned seed) {
    unsigned a[8];
    for (int i = 0; i < 8; ++i) a[i] = threadIdx.x * 2654435761u + i * 40503u + seed;
    unsigned b = seed | 0x01020304u;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int rep = 0; rep < 4; ++rep)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (OP == 0) a[i] = __builtin_amdgcn_udot4(a[i], b, a[(i + 3) & 7], false);
                if (OP == 1) a[i] = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, a[i]), __builtin_bit_cast(us2, b), a[(i + 3) & 7], false);
                if (OP == 2) a[i] = __builtin_amdgcn_perm(a[i], a[(i + 3) & 7], b);
                if (OP == 3) a[i] = __builtin_amdgcn_alignbyte(a[i], a[(i + 3) & 7], 1);
                if (OP == 4) a[i] = a[i] * 18u + a[(i + 3) & 7];                       // v_mad_u32_u24 or v_mul_lo + add
                if (OP == 5) a[i] = (a[i] >> 3) | (a[(i + 3) & 7] << 16);                 // v_lshl_or / alignbit
                if (OP == 6) a[i] = (unsigned)__builtin_amdgcn_update_dpp((int)a[(i + 3) & 7], (int)a[i], 0x138, 0xf, 0xf, false);
                if (OP == 7) a[i] = a[i] + a[(i + 3) & 7];
                if (OP == 8) a[i] = min(a[i], a[(i + 3) & 7]) ^ b;                         // 2 ops
                if (OP == 9) { float f = __builtin_bit_cast(float, a[i]); f = __builtin_fmaf(f, 1.0001f, 0.5f); a[i] = __builtin_bit_cast(unsigned, f); }
                if (OP == 10) a[i] = __shfl_up(a[i], 1, 64);
                // the packed 16-bit forms of k_fast_cells (csrc/fast_forms.hpp) and what they stand beside
                const unsigned o = a[(i + 3) & 7];
                if (OP == 11) a[i] = __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(ss2, a[i]), __builtin_bit_cast(ss2, o)));
                if (OP == 12) a[i] = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(ss2, a[i]), __builtin_bit_cast(ss2, o)));
                if (OP == 13) a[i] = __builtin_bit_cast(unsigned, __builtin_bit_cast(ss2, a[i]) - __builtin_bit_cast(ss2, o));
                if (OP == 14) a[i] = __builtin_bit_cast(unsigned, __builtin_elementwise_sub_sat(__builtin_bit_cast(us2, a[i]), __builtin_bit_cast(us2, o)));
                if (OP == 15) asm volatile("v_max_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:BYTE_2" : "=v"(a[i]) : "v"(a[i]), "v"(o));
                if (OP == 16) a[i] = __builtin_amdgcn_alignbit(a[i], o, 5);
                if (OP == 17) asm volatile("v_and_or_b32 %0, %1, %2, %3" : "=v"(a[i]) : "v"(a[i]), "v"(b), "v"(o));
                if (OP == 18) a[i] = __builtin_bit_cast(unsigned, __builtin_bit_cast(ss2, a[i]) * __builtin_bit_cast(ss2, b) + __builtin_bit_cast(ss2, o));
                if (OP == 19) a[i] = __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(ss2, a[i]), __builtin_shufflevector(__builtin_bit_cast(ss2, o), __builtin_bit_cast(ss2, o), 1, 0)));
                if (OP == 20) asm volatile("v_pk_lshrrev_b16 %0, 15, %1 op_sel_hi:[0,1]" : "=v"(a[i]) : "v"(o));
            }
    }
    unsigned s = 0;
    for (int i = 0; i < 8; ++i) s ^= a[i];
    out[blockIdx.x * 512 + threadIdx.x] = s;
}
template <int OP> void run(const char* name, unsigned* d, int per_iter) {
    const int blocks = 256 * 4, iters = 2000;   // 4 blocks of 8 waves per CU: 8 waves per SIMD
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL(k<OP>, dim3(blocks), dim3(512), 0, 0, d, 10, 1u);
    hipEventRecord(e0);
    hipLaunchKernelGGL(k<OP>, dim3(blocks), dim3(512), 0, 0, d, iters, 1u);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    const double wave_instr = (double)blocks * 8 * iters * 32 * per_iter;     // per launch
    const double per_simd = wave_instr / (256.0 * 4);
    printf("%-28s %8.3f ms  -> %.2f ns per wave-instruction per SIMD (%.2f cycles at 2.4 GHz)\n", name, ms, ms * 1e6 / per_simd, ms * 1e6 / per_simd * 2.4);
}
int main() {
    unsigned* d; hipMalloc(&d, 256 * 4 * 512 * 4);
    run<9>("v_fma_f32", d, 1); run<7>("v_add_u32", d, 1); run<0>("v_dot4_u32_u8", d, 1); run<1>("v_dot2_u32_u16", d, 1); run<2>("v_perm_b32", d, 1);
    run<3>("v_alignbyte_b32", d, 1); run<4>("mul + add (u32)", d, 1); run<5>("shift | shift", d, 1); run<6>("v_mov_dpp wave_shr:1", d, 1); run<8>("min, xor (2 ops)", d, 2);
    run<10>("__shfl_up(., 1)", d, 1);
    run<11>("v_pk_min_i16", d, 1); run<12>("v_pk_max_i16", d, 1); run<13>("v_pk_sub_i16", d, 1); run<14>("v_pk_sub_u16 clamp", d, 1);
    run<15>("v_max_u32_sdwa (byte sel)", d, 1); run<16>("v_alignbit_b32", d, 1); run<17>("v_and_or_b32", d, 1); run<18>("v_pk_mad_u16", d, 1);
    run<19>("v_pk_min_i16 op_sel swap", d, 1); run<20>("v_pk_lshrrev_b16", d, 1);
    return 0;
}
