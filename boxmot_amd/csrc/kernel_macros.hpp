// Spellings of the few gfx950 constructs the kernels use through a macro so that the test harness
// (tests/host_emu) can substitute an instrumented equivalent when it executes the same source on
// CPU threads.  In the product build these are exactly the HIP builtins below.
#pragma once

#ifndef BM_DYNAMIC_LDS_T
// dynamic LDS of the workgroup; keep the base 16-byte aligned (DS b64/b128 accesses)
#define BM_DYNAMIC_LDS_T(type, name) extern __shared__ __attribute__((aligned(16))) type name[]
#endif
#ifndef BM_EXPF
#define BM_EXPF(x) __expf(x)
#endif
#ifndef BM_MFMA_F16_K16
#define BM_MFMA_F16_K16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0)
#define BM_MFMA_F16_K32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0)
#endif
#ifndef BM_SCHED_FENCE
// compile-time scheduling fence: keeps the per-tile register working set from being merged
// across tiles by the instruction scheduler (which otherwise hoists every LDS read and spills)
#define BM_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#endif
#ifndef BM_OPAQUE_U32
// makes a value opaque to the optimiser (defeats loop-invariant hoisting of the loads that depend on it)
#define BM_OPAQUE_U32(x) asm volatile("" : "+v"(x))
#endif
#ifndef BM_ROW_SHL1_F32
// neighbour exchange inside each row of 16 lanes as DPP modifiers (no LDS crossbar traffic): the value of
// lane+1 / lane-1 (0 where the row has no such lane) / lane-1 with wrap-around
#define BM_DPP_F32(v, ctrl) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, (float)(v)), ctrl, 0xf, 0xf, true))
#define BM_ROW_SHL1_F32(v) BM_DPP_F32(v, 0x101)
#define BM_ROW_SHR1_F32(v) BM_DPP_F32(v, 0x111)
#define BM_ROW_ROR1_F32(v) BM_DPP_F32(v, 0x121)
#endif
#ifndef BM_DPP_U32
// raw DPP move: lanes whose source lane does not exist take 0 (zero_fill) or keep `old`
#define BM_DPP_U32(old, v, ctrl, zero_fill) ((unsigned)__builtin_amdgcn_update_dpp((int)(old), (int)(v), ctrl, 0xf, 0xf, zero_fill))
#endif
#ifndef BM_READLANE_U32
// the value a given (compile-time) lane holds, as a wave-uniform scalar
#define BM_READLANE_U32(v, l) ((unsigned)__builtin_amdgcn_readlane((int)(v), l))
#endif
#ifndef BM_WAVE_SUM_F32
// Sum over the 64 lanes with the value (and the rounding) of the xor butterfly v += shfl_xor(v, 1), 2, 4, 8, 16, 32, on the DPP
// path instead of six LDS-crossbar round trips: quad swaps (quad_perm 1,0,3,2 and 2,3,0,1), then mirrors -- after the quad steps
// the lanes of a quad agree, so l <-> 7 - l (row_half_mirror) and l <-> 15 - l (row_mirror) add what l ^ 4 and l ^ 8 would; the
// four rows meet as (S0 + S1) + (S2 + S3), the value every lane of the butterfly ends with (fp32 addition commutes).
#define BM_DPP_F32_RAW(v, ctrl) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, (float)(v)), ctrl, 0xf, 0xf, true))
__device__ inline float bm_wave_sum_f32(float v) {
    v += BM_DPP_F32_RAW(v, 0xB1); v += BM_DPP_F32_RAW(v, 0x4E); v += BM_DPP_F32_RAW(v, 0x141); v += BM_DPP_F32_RAW(v, 0x140);
    const int b = __builtin_bit_cast(int, v);
    const float s0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)), s1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16)),
                s2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)), s3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
    return (s0 + s1) + (s2 + s3);
}
#define BM_WAVE_SUM_F32(v) bm_wave_sum_f32(v)
#endif
#ifndef BM_WAVE_LDS_SYNC
// LDS written by some lanes of a wavefront and read by others of the SAME wavefront: the DS operations of one wave execute in
// order, so only the compiler has to be kept from reordering them (no workgroup barrier)
#define BM_WAVE_LDS_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
#endif
#ifndef BM_GLDS16
// asynchronous 16-byte global -> LDS copy (global_load_lds_dwordx4): every lane names its own global source, the LDS
// destination is the wave-uniform `lds_wave_base` + 16 * lane.  Completion is tracked by vmcnt (a following __syncthreads()
// drains it).
#define BM_GLDS16(gptr, lds_wave_base, lane) \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gptr), \
                                     (__attribute__((address_space(3))) void*)(lds_wave_base), 16, 0, 0)
#endif
#ifndef BM_GLDS4
// the 4-byte form (global_load_lds_dword): LDS destination `lds_wave_base` + 4 * lane
#define BM_GLDS4(gptr, lds_wave_base, lane) \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gptr), \
                                     (__attribute__((address_space(3))) void*)(lds_wave_base), 4, 0, 0)
#endif
#ifndef BM_WAIT_VM0
// wait for this wave's outstanding vector-memory operations, BM_GLDS16 copies included: the compiler does not order a
// global -> LDS copy against a later workgroup barrier, so the wave that issued copies waits here before the barrier that
// publishes them (s_waitcnt vmcnt(0); vmcnt retires in order)
#define BM_WAIT_VM0() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#endif
#ifndef BM_RESID_F16
// v - (float)(fp16 half `hi` of the packed pair `hp`): one v_fma_mix_f32 (fma(h, -1.0, v): a single rounding, i.e. the fp32
// subtraction itself) instead of a convert + a subtract
#define BM_RESID_F16(hp, hi, v, out) asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[" #hi ",0,0] op_sel_hi:[1,0,0]" : "=v"(out) : "v"(hp), "v"(v))
#endif
#ifndef BM_RELU_F32
// max(v, 0) as one integer max on the bit pattern (negative floats are negative ints); a float max costs a second,
// canonicalising v_max under IEEE mode
#define BM_RELU_F32(v) __builtin_bit_cast(float, __builtin_elementwise_max(__builtin_bit_cast(int, (float)(v)), 0))
#endif
#ifndef BM_QUAD_SWAP1_F32
// value of the horizontally adjacent lane (lane ^ 1) as a DPP quad permute [1,0,3,2]
#define BM_QUAD_SWAP1_F32(v) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, (float)(v)), 0xB1, 0xf, 0xf, true))
#endif
#ifndef BM_UNIFORM_I32
// a value that is the same in every lane of the wavefront (e.g. the wave index), moved to a scalar register so that
// everything derived from it (ring-buffer modulo, row offsets, base pointers) is computed once on the scalar unit
#define BM_UNIFORM_I32(x) __builtin_amdgcn_readfirstlane((int)(x))
#endif
#ifndef BM_MUL24
// unsigned multiplies of operands that fit 24 bits: the full-rate v_mul_u32_u24 / v_mul_hi_u32_u24 instead of the quarter-rate
// 32-bit multiplies the compiler must pick when it cannot see the ranges (BM_MULHI24 = bits 32.. of the 48-bit product)
#define BM_MUL24(a, b) ((unsigned)__umul24((unsigned)(a), (unsigned)(b)))
__device__ inline unsigned bm_mulhi24(unsigned a, unsigned b) {
    unsigned d;
    asm("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
#define BM_MULHI24(a, b) bm_mulhi24((unsigned)(a), (unsigned)(b))
#endif
#ifndef BM_CLOCK
#define BM_CLOCK() wall_clock64()
#endif
#ifndef BM_LDS_FLAG_SET
// Wave-to-wave progress flags in LDS: neighbour synchronisation where a workgroup barrier would make eight waves wait for the
// slowest.  The DS operations of ONE wave are executed in order by the LDS unit, so a flag stored after data stores becomes visible
// after them, and a wave that has seen the flag reads the data with later (in-order) DS reads; the `memory` clobbers keep the
// compiler from moving LDS accesses across either side.  The wait polls (s_sleep between polls) until *flag >= value and is BOUNDED:
// a broken protocol must produce wrong numbers in a test, never a hung GPU -- after BM_LDS_SPIN_LIMIT polls it gives up.
#define BM_LDS_SPIN_LIMIT (1 << 18)
// (the flags are addressed as LDS -- ds_write_b32 / ds_read_b32 -- not through generic pointers: a flat access would also wait for
// the wave's outstanding GLOBAL loads, i.e. for the weight fragments prefetched a layer ahead)
typedef __attribute__((address_space(3))) int bm_lds_int_t;
#define BM_LDS_FLAG_SET(ptr, val) do { asm volatile("" ::: "memory"); *(volatile bm_lds_int_t*)(ptr) = (val); asm volatile("" ::: "memory"); } while (0)
__device__ inline bool bm_lds_flag_wait(const volatile bm_lds_int_t* p, int v) {
    bool ok = false;
#pragma unroll 1
    for (int k = 0; k < BM_LDS_SPIN_LIMIT; ++k) {
        if (__builtin_amdgcn_readfirstlane(*p) >= v) { ok = true; break; }       // wave-uniform: one scalar branch per poll
        __builtin_amdgcn_s_sleep(2);
    }
    asm volatile("" ::: "memory");
    return ok;
}
#define BM_LDS_FLAG_WAIT(ptr, val) bm_lds_flag_wait((const volatile bm_lds_int_t*)(ptr), (val))
#endif

// wave priority around an MFMA burst (s_setprio) and the hardware reciprocal (v_rcp_f32, 1 ulp)
#ifndef BM_SETPRIO
#define BM_SETPRIO(n) __builtin_amdgcn_s_setprio(n)
#endif
#ifndef BM_RCPF
#define BM_RCPF(x) __builtin_amdgcn_rcpf(x)
#endif

// fp32 matrix pipe: D = A.B + C on 16x16x4 tiles (v_mfma_f32_16x16x4_f32; A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15],
// D: column lane & 15, rows 4 (lane >> 4) + r).  Exact fp32: bit-for-bit the k-ordered fmaf chain, so a kernel written on it
// returns what the same sums written as scalar fmaf loops return (the test harness substitutes exactly that).
#if defined(__clang__)
typedef float bm_f4 __attribute__((ext_vector_type(4)));
#else
typedef float bm_f4 __attribute__((vector_size(16)));
#endif
#ifndef BM_MFMA_F32_K4
#define BM_MFMA_F32_K4(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0)
#endif
