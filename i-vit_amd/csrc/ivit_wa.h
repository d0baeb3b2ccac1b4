// ivit_wa.h — the device idioms of the "weights as the A operand" kernels, written once.  The family: mlp384rs_kernel
// (ivit_mlp_rs.h), swin_mlp_rs_kernel (ivit_swin_mlp_rs.h), gemm_wreg_kernel (ivit_gemm_wreg.h), gemm_ws_qkv_kernel (ivit_gemm_ws.h).
//
// The scheme they share: v_mfma_i32_32x32x32_i8 with the weights as the A operand (rows = channels) and 32 tokens as the B operand
// (a lane = a token).  The rows of a weight fragment are placed so that MFMA row q*8 + h*4 + i is channel h*16 + q*4 + i of the
// 32-channel tile (wa_chan_of_row): accumulator register v of lane (token, h) is then channel 16 h + v — sixteen CONSECUTIVE
// channels per lane, requantised by the fp64 magic number (ivit_device.h: RQ_MAGIC, rq_magic), packed by the saturating packs
// and stored 16 bytes at a time straight from registers.
//
// Nothing here owns scheduling: waits, look-ahead distances, scheduling fences and store predicates stay in the kernel that calls
// it, and each kernel compiles to the instruction stream it had with its own copy of the text.  That is also what decides the
// form of each piece: a force-inlined function where that holds, a macro where only the written-out text does (each says so).
#pragma once
#include <type_traits>
#include "ivit_device.h"

// channel (of its 32-channel tile) held by MFMA row rho: plan-time swizzles and register-resident weight loads place row
// q*8 + h*4 + i at channel h*16 + q*4 + i
__device__ __forceinline__ int wa_chan_of_row(int rho) { return ((rho >> 2) & 1) * 16 + (rho >> 3) * 4 + (rho & 3); }
// LDS images [64-column block][token][64 B]: the four 16-byte chunks of a token's 64 B are permuted by
// g(token) = ((token >> 1) & 3) ^ gray((token >> 3) & 3): conflict-free both for the B-fragment ds_read_b128 (lane groups
// {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and their upper-half twins: MI355X_MICROARCH.md, LDS) and for a producer's
// ds_write_b128 (eight consecutive tokens per group, 32 banks)
__device__ __forceinline__ int wa_g(int tok) { return ((tok >> 1) & 3) ^ ((tok >> 3) & 3) ^ ((tok >> 4) & 1); }

// ---- hand-over by monotonically increasing LDS counters (the role-split kernels: no workgroup barrier after the prologue).  An LDS
// instruction stream of one wave executes in order, so "data accesses, then ds_add" / "ds_read counter, then data accesses" need no
// fences beyond keeping the compiler from reordering them (asm volatile + memory clobber).
// Both primitives are single asm blocks: straight-line code for the register allocator (as C++ the spin loop was
// unrolled nine times and every `if (lane == 0)` split a basic block: 1.4 K spilled registers in the producers).
__device__ __forceinline__ void rs_signal(unsigned flag_addr) {            // lane 0 adds 1 (flag_addr is wave-uniform)
    unsigned long long save;
    asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, 1\n\tds_add_u32 %1, %2\n\ts_mov_b64 exec, %0"
                 : "=&s"(save) : "v"(flag_addr), "v"(1u) : "memory");
}
// spin until the LDS counter reaches `target` (the counters only grow).  A hand-over that never comes is a bug: trap loudly —
// after 2^28 polls of >= 64 cycles each (~10 s: far beyond any stall a debugger, a profiler or throttled clocks produce, short
// enough that a real deadlock ends the launch instead of wedging the queue)
__device__ __forceinline__ void rs_wait(unsigned flag_addr, unsigned target) {
    unsigned v, cnt, tmp;
    asm volatile("s_mov_b32 %1, 0\n"
                 ".Lrsw%=:\n\t"
                 "ds_read_b32 %0, %3\n\t"
                 "s_waitcnt lgkmcnt(0)\n\t"
                 "v_readfirstlane_b32 %2, %0\n\t"
                 "s_sub_i32 %2, %2, %4\n\t"
                 "s_cmp_ge_i32 %2, 0\n\t"
                 "s_cbranch_scc1 .Lrsd%=\n\t"
                 "s_sleep 1\n\t"
                 "s_add_u32 %1, %1, 1\n\t"
                 "s_cmp_lt_u32 %1, 0x10000000\n\t"
                 "s_cbranch_scc1 .Lrsw%=\n\t"
                 "s_trap 2\n"
                 ".Lrsd%=:"
                 : "=&v"(v), "=&s"(cnt), "=&s"(tmp) : "v"(flag_addr), "s"(target) : "memory", "scc");
}

// ---- four int32 -> one dword of BIASED bytes: o = Q + 128 comes out of the requant (magic + 128 in the low dword);
// v_cvt_pk_i16_i32 and v_sat_pk_u8_i16 saturate to [0, 255] = clamp(Q, -128, 127) + 128 while packing.  A consumer that wants
// two's-complement bytes takes the bias off with one xor (0x80808080) per dword; ShiftGELU's table is indexed by the biased byte
__device__ __forceinline__ unsigned wa_pack_biased(int o0, int o1, int o2, int o3) {
    unsigned p01, p23, b01, b23;
    asm("v_cvt_pk_i16_i32 %0, %1, %2" : "=v"(p01) : "v"(o0), "v"(o1));
    asm("v_cvt_pk_i16_i32 %0, %1, %2" : "=v"(p23) : "v"(o2), "v"(o3));
    asm("v_sat_pk_u8_i16 %0, %1" : "=v"(b01) : "v"(p01));
    asm("v_sat_pk_u8_i16 %0, %1" : "=v"(b23) : "v"(p23));
    return __builtin_amdgcn_perm(b23, b01, 0x05040100u);
}

// ---- an accumulator that starts at the bias: the lane's sixteen consecutive channels as four 16-byte loads.  B4_Q: the v4i of
// channels 4 q .. 4 q + 3 as an expression in `q` (a global or LDS pointer, or an LDS byte address).  A macro: as a force-inlined
// function (v16i returned, or filled by reference) the same four loads reach the back end in another order — gemm_wreg_kernel's
// prologue is scheduled differently — while this text compiles to the streams the kernels had with the loop written out
#define WA_ACC_BIAS(acc, B4_Q)                                                                                          \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                                     \
        const v4i b4_ = B4_Q;                                                                                           \
        acc[4 * q] = b4_[0]; acc[4 * q + 1] = b4_[1]; acc[4 * q + 2] = b4_[2]; acc[4 * q + 3] = b4_[3];                 \
    }

// ---- 16-bit requant + the block's residual QuantAct (quant_utils.py:232-245), one output dword = two channels at a time:
//   clamp16(rq(identity, cr) + rq(clamp16(rq(acc, c)), cm)) of channels 2 d (a0, c2[0], low half of rw) and 2 d + 1, packed.
// RQ: the form of the first requant (rq_magic: 1 one FMA, 0 multiply then add, 2 v_rndne_f64 + saturating convert).  rw: the identity
// branch's two 16-bit values.  res_fast: std::true_type where the host proved |cm|, |cr| < RQ_FAST_CLIM, else a bool decided in the
// kernel.  Both terms of the sum are integers < 2^31 / 2: the sum is the reference's fp64 sum; v_cvt_pk_i16_i32 clamps to 16 bits
// while packing.  Scalars by value, a dword at a time: the form that takes the lane's whole accumulator and identity rows (by
// reference or by value) changes the order of the identity loads in its callers.  The caller keeps the loop over its eight dwords,
// where its multipliers come from, and its store predicate
template <int RQ, typename RF>
__device__ __forceinline__ int wa_res_pair(int a0, int a1, v2d c2, int rw, double cm, double cr, RF res_fast) {
    int o[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int t16 = min(max(rq_magic<RQ>(h ? a1 : a0, c2[h]), -32768), 32767);
        const int r = h ? (rw >> 16) : (int)(short)(rw & 0xffff);
        if constexpr (std::is_same<RF, std::true_type>::value) o[h] = rq_fast(r, cr) + rq_fast(t16, cm);
        else o[h] = res_fast ? rq_fast(r, cr) + rq_fast(t16, cm) : rq_magic<2>(r, cr) + rq_magic<2>(t16, cm);
    }
    int pk;
    asm("v_cvt_pk_i16_i32 %0, %1, %2" : "=v"(pk) : "v"(o[0]), "v"(o[1]));
    return pk;
}

// ---- ShiftGELU (+ qact1) by table, one hidden dword (four biased bytes) at a time: the byte's value is the index into the token's
// 256-byte table line at LDS address `base` (256-aligned, so base | byte is the address: one SDWA each).  Two halves, so that the
// caller decides how far the gathers run ahead of the merge and which s_waitcnt stands between them:
//   issue: four addresses, four byte gathers into g[0..3] (asm volatile: they stay in this order, behind the table line's write);
//   merge: the four gathered bytes -> the dword that replaces w.  Must follow a wait that covers the gathers of g.
// ds_read_u8_d16_hi returns byte << 16 with the low half ZEROED, the d16 behaviour of SRAM-ECC parts (the only mode MI355X ships
// in; i-vit_amd/_lib.py); a target without it would need the merge written out
__device__ __forceinline__ void wa_gelu_issue(unsigned w, unsigned base, unsigned (&g)[4]) {
    unsigned a0, a1, a2, a3;
    asm("v_or_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD" : "=v"(a0) : "v"(w), "v"(base));
    asm("v_or_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD" : "=v"(a1) : "v"(w), "v"(base));
    asm("v_or_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(a2) : "v"(w), "v"(base));
    asm("v_or_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(a3) : "v"(w), "v"(base));
    asm volatile("ds_read_u8 %0, %1" : "=v"(g[0]) : "v"(a0) : "memory");
    asm volatile("ds_read_u8 %0, %1" : "=v"(g[1]) : "v"(a1) : "memory");
    asm volatile("ds_read_u8_d16_hi %0, %1" : "=v"(g[2]) : "v"(a2) : "memory");
    asm volatile("ds_read_u8_d16_hi %0, %1" : "=v"(g[3]) : "v"(a3) : "memory");
}
__device__ __forceinline__ unsigned wa_gelu_merge(const unsigned (&g)[4]) {
    unsigned o, t13;
    asm volatile("v_or_b32 %0, %1, %2" : "=v"(t13) : "v"(g[1]), "v"(g[3]));      // volatile: behind the caller's wait
    asm volatile("v_or3_b32 %0, %1, %2, %3" : "=v"(o) : "v"(g[0]), "v"(g[2]), "v"(t13 << 8));
    return o;
}

// ---- one token group of an activation tile, global -> LDS by DMA: 16 tokens x 4 chunk slots per global_load_lds, one instruction
// per 64-column block.  The image [KB blocks][tokens][64 B] starts at sm + IMG, KBLK bytes per block; token group tg holds rows
// ROW0 + 16 tg ... (clamped to M - 1: a short tile holds defined bytes) of x [M][64 KB].  The chunk permutation is applied on the
// source side — the source chunk of a slot is slot ^ g(token) — because the LDS side of a DMA is lane-linear.  A macro: as a
// force-inlined function taking `sm`, the piece's scalar address arithmetic (tg * 1024 and what follows from it) is placed and
// scheduled differently in gemm_ws_qkv_kernel; this text compiles to the stream each kernel had with the loop written out
#define WA_DMA16(KB, KBLK, sm, IMG, tg, lane, x, ROW0, M)                                                               \
    {                                                                                                                   \
        const int tokl = (tg) * 16 + ((lane) >> 2), c = ((lane) & 3) ^ wa_g(tokl);                                      \
        const long long grow = min((ROW0) + tokl, (long long)(M) - 1);                                                  \
        const int8_t *src = (x) + grow * ((KB) * 64) + c * 16;                                                          \
        _Pragma("unroll") for (int kb = 0; kb < (KB); ++kb) {                                                           \
            const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)((IMG) + kb * (KBLK) + (tg) * 1024));         \
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + kb * 64),          \
                                             (__attribute__((address_space(3))) void *)((sm) + dst), 16, 0, 0);         \
        }                                                                                                               \
    }
