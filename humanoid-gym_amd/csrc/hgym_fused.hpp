// hgym_fused.hpp -- the bf16 fast path of the actor / critic (/ auxiliary head): three kernels that replace ~70 launches per minibatch.
//
//   mlp_fwd_kernel<BM>   gather + fp32->bf16 + Linear/ELU x3 + head (+ Gaussian sample / log-prob) for a tile of BM rows;
//                        activations never leave the CU between layers (LDS), weights stream from L2 straight into
//                        MFMA operand registers.  Used by the rollout (PPO.act, BM = 32; hgym_rollout.hip puts the env step of
//                        the tile's 32 envs behind it in the same launch) and for inference.
//   mlp_fb_kernel        the update: the same forward on 64-row tiles, the loss gradient on the head wavefronts (PPO surrogate /
//                        value loss / the auxiliary head's MSE) and dZ_l = (dZ_{l+1} * W_{l+1}) .* elu'(H_l) for l = 2, 1, 0 on the
//                        activations still resident in LDS; one grid row per net.  (mlp_fb_head_kernel: the actor's tile with a
//                        head of its own -- the mirror loss, the smoothness regulariser, behaviour cloning.)
//   dw_kernel_rs         all weight-gradient products dW_l = dZ_l^T * X_l (+ bias gradients) in ONE launch:
//                        contraction over the batch, operands staged registers -> LDS and read with the gfx950
//                        transpose read (ds_read_b64_tr_b16), so no transposed copy of anything exists in HBM.
//
// Activation layout ("block layout", global and LDS alike): a (rows x cols) bf16 matrix is stored as 16x16 blocks,
// block (mb, cb) at ((mb * CB + cb) * 512) bytes, row-major inside the block (32 B per row).  With it
//   * an MFMA 16x16x32 operand fragment (lane l: row l&15, k-chunk l>>4) is one ds_read_b128 per lane, bank-conflict
//     free (rows 32 B apart, chunk pairs 512 B apart);
//   * an MFMA epilogue (lane l: row l&15, 4 consecutive columns 4*(l>>4)..) writes one 512-byte block per wave
//     instruction, to LDS and to HBM, fully coalesced;
//   * the transpose read of the weight-gradient kernel is lane-linear (address = block + 8 * lane).
// Weight operand layout: "fragment-major", fragment (nb, kb) = 1 KiB in exact lane order (lane l: row nb*16 + (l&15),
// k = kb*32 + 8*(l>>4) .. +7), so a wavefront's weight load is one contiguous 1 KiB global_load_dwordx4.
#pragma once
#include <type_traits>

#include "hgym_finalize.hpp"
// This header's arithmetic is compiled with the same contraction setting in every translation unit (hgym_net.hip: the default;
// hgym_rollout.hip: built with -ffp-contract=off for the env arithmetic it also contains, and defines HGYM_TU_CONTRACT_OFF).
#pragma clang fp contract(fast)
#include "hgym_gemm.hpp"

namespace hgym {

constexpr int FUSED_CHUNK = 128;      // input columns staged per first-layer chunk (4 k-blocks of 32)
// HGYM_L0_TRIM: which first-layer loops stop at FusedLayer::KR instead of KB (A/B builds): 0 none, 1 the tiles with a ring of 4
// (32-row tiles), 2 all
#ifndef HGYM_L0_TRIM
#define HGYM_L0_TRIM 2
#endif
// Workgroup shapes: the update uses 64-row tiles with 16 wavefronts (4 per SIMD: the weight stream comes from L2 with
// ~1 us latency under load and only thread-level parallelism hides it); the rollout uses 32-row tiles with 8 wavefronts,
// two workgroups per CU.

struct __attribute__((packed, aligned(4))) F4 {
    float v[4];
};
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

struct FusedLayer {
    const u32x4* Wf;    // forward fragments  [NB][KB][64] x 16 B
    const u32x4* WTf;   // backward fragments [K/16][NBB][64] x 16 B (this layer's W, transposed role)
    const float* bias;  // [N] fp32, 4-byte aligned
    int K, N;           // logical in / out features
    int KB;             // forward contraction blocks of 32 the fragment buffer holds (first layer: padded to whole 128-column chunks)
    int NB;             // forward output blocks of 16
    int NBB;            // backward contraction blocks of 32 (N padded to 32)
    int KR;             // forward contraction blocks that hold a valid column, ceil(K / 32) <= KB: the k-steps a first-layer loop runs
};

// First layer of width K: what the buffers hold and what the loops run.  The weight fragments, the bf16 shadow and X0 are padded to
// whole chunks (KB k-steps, NC chunks of 4); k-steps [KR, KB) hold zero weights against zero input columns and add +0 to
// accumulators that started from +0, so the loops stop at KR: the last chunk runs nlast = KR - 4 (NC - 1) k-steps (1..4).
struct L0KSteps {
    int KB, KR, NC, nlast;
};
inline L0KSteps l0_ksteps(int K) {
    L0KSteps s;
    s.KB = (K + FUSED_CHUNK - 1) / FUSED_CHUNK * (FUSED_CHUNK / 32);
    s.KR = (K + 31) / 32;
    s.NC = s.KB / 4;
    s.nlast = s.KR - 4 * (s.NC - 1);
    return s;
}

struct FusedNet {
    FusedLayer layer[4];
    const float* x;     // fp32 input rows (observations), leading dimension ldx
    int64_t ldx;
    // bf16 shadow of the input rows: row-major, leading dimension a multiple of 8 and >= 32 * layer[0].KB, pad columns zero.
    //   xb != null (XB16 instantiations): the first layer gathers ITS INPUT from here -- 2 B per element, no conversion, and
    //              the weight-gradient kernel gathers the same rows again by index, so no X0 copy is written at all;
    //   xs != null (fp32-input instantiations, no row gather): the tile also stores the bf16 it has just formed for LDS as row
    //              m of this array -- how the rollout's policy launches leave the shadow of every storage slot behind.
    const __bf16* xb;
    int64_t ldxb;
    __bf16* xs;
    int64_t ldxs;
    __bf16* X0;         // bf16 copy of the gathered input, block layout, CB = 2 * layer[0].KB   (train only)
    __bf16* H[3];       // hidden activations, block layout, CB = layer[l].N / 16                 (train only)
    __bf16* dZ[4];      // pre-activation gradients; dZ[3] (32 * layer[3].NBB columns) is written by the loss kernel
    float* out;         // fp32 head output (M, layer[3].N) row-major
    int64_t ldo;
};

HG_HD int fused_lds_p(const FusedNet& n, int BM) { return BM * (n.layer[0].N > n.layer[2].N ? n.layer[0].N : n.layer[2].N) * 2; }
// fp32 copies of the four bias vectors (fetched at kernel entry so no epilogue waits on a cold global load) + 16 pad
HG_HD int fused_lds_bias(const FusedNet& n) { return (n.layer[0].N + n.layer[1].N + n.layer[2].N + 16 * n.layer[3].NB + 16) * 4; }
HG_HD int fused_lds_q(const FusedNet& n, int BM) {
    const int a = 2 * BM * FUSED_CHUNK * 2, b = BM * n.layer[1].N * 2;
    return a > b ? a : b;
}

__device__ __forceinline__ u32x2 pack_bf16x4(float a, float b, float c, float d) {
    typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
    bf16x4 v = {(__bf16)a, (__bf16)b, (__bf16)c, (__bf16)d};
    return __builtin_bit_cast(u32x2, v);
}
// Streaming accesses (data touched once per launch) carry the non-temporal hint so that they do not push the weight
// fragments, which every workgroup re-reads, out of the XCD's L2: kFusedNT bit 0 = input gather loads, bit 1 = X0 / H stores
// of the forward, bit 2 = H loads / dZ stores of the dZ chain.  Same-box A/B per minibatch (B = 61 440, storage 245 760 rows):
// forward 265.6 -> 257.6..262.8 us (bit 0 alone 255), dZ chain 134.4 -> 127.5 us, dW (reads what those wrote) 185 -> 181 us.
constexpr int kFusedNT = 7;
typedef f32x4 f32x4_u4 __attribute__((aligned(4)));
template <bool NT>
__device__ __forceinline__ F4 ld_stream_f4(const float* p) {
    if (NT) return __builtin_bit_cast(F4, __builtin_nontemporal_load(reinterpret_cast<const f32x4_u4*>(p)));
    return *reinterpret_cast<const F4*>(p);
}
template <bool NT>
__device__ __forceinline__ void st_stream_u2(char* p, u32x2 v) {
    if (NT) __builtin_nontemporal_store(v, reinterpret_cast<u32x2*>(p));
    else *reinterpret_cast<u32x2*>(p) = v;
}
template <bool NT>
__device__ __forceinline__ u32x2 ld_stream_u2(const char* p) {
    if (NT) return __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
    return *reinterpret_cast<const u32x2*>(p);
}
template <bool NT>
__device__ __forceinline__ u32x4 ld_stream_u4(const char* p) {
    if (NT) return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    return *reinterpret_cast<const u32x4*>(p);
}
__device__ __forceinline__ float bf16_bits_to_f32(unsigned int lo16) { return __builtin_bit_cast(float, lo16 << 16); }

// Epilogue stores, 16 bytes per lane.  An MFMA epilogue lane (r = lane & 15, q = lane >> 4) holds 4 consecutive bf16 columns of row r of a
// 16 x 16 block: 8 bytes at r * 32 + q * 8, so the natural store is one dwordx2 per block -- and the update's tiles turned out to be
// paced by store ISSUE (round 4: without its H / dZ stores mlp_fb2_kernel ran 271 instead of 440 us on a slow-class box; MI355X_MICROARCH.md:
// a dwordx2 store tail moves ~7 B/clk/CU, dwordx4 twice that).  For TWO blocks A and B (same lane offsets), v_permlane16_swap_b32 exchanges
// the odd 16-lane rows of A's register with the even rows of B's: afterwards a lane with q even holds columns 8 (q / 2) .. + 7 of row r of
// block A (its own 8 bytes and its right neighbour's), a lane with q odd the same of block B -- one dwordx4 per lane for the pair, same
// bytes, same addresses, half the store instructions.  HGYM_WIDE_ST=0 restores the dwordx2 form (A/B builds).
template <bool NT>
__device__ __forceinline__ void st_stream_u4(char* p, u32x4 v) {
    if (NT) __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
    else *reinterpret_cast<u32x4*>(p) = v;
}
// pa / pb: block A / B base + this lane's r * 32 + q * 8; oka / okb: whether block A / B is stored at all (wave-uniform)
template <bool NT, bool WIDE = true>
__device__ __forceinline__ void st_pair(char* pa, char* pb, u32x2 a, u32x2 b, bool oka, bool okb, int q) {
    if constexpr (!WIDE) {
        if (oka) st_stream_u2<NT>(pa, a);
        if (okb) st_stream_u2<NT>(pb, b);
        return;
    }
    const auto s0 = __builtin_amdgcn_permlane16_swap(a[0], b[0], false, false);
    const auto s1 = __builtin_amdgcn_permlane16_swap(a[1], b[1], false, false);
    const u32x4 v = {s0[0], s1[0], s0[1], s1[1]};
    const bool odd = q & 1;
    char* p = odd ? pb - 8 : pa;
    if (odd ? okb : oka) st_stream_u4<NT>(p, v);
}

// ---- weight stream ------------------------------------------------------------------------------------------------------
// The weight fragments of one output strip (G n-blocks) stream from L2 into a register ring of D k-steps per wavefront:
// slot t % D holds k-step t, and the slot is re-loaded with k-step t + D as soon as its MFMAs have been issued, so D - 1
// k-steps of loads (D * G KiB per wavefront) are in flight under the MFMAs of one.  L2 latency under load is ~1 us and the
// MFMAs of a k-step take ~0.1 us: a ring primed ONE layer (or one strip) ahead -- before the epilogue and the barrier of the
// previous one -- never starts cold.  D = 4 for the 8-wave rollout tiles (2 waves per SIMD, 256 VGPRs each), D = 2 for the
// 16-wave update tiles (4 waves per SIMD hide the rest).
template <int G, int D>
struct WRing {
    u32x4 w[D][G];
};

// issue the loads of k-steps [0, min(D, nk)) of the stream whose fragment (g, t) is wl[g * wstride + t * 64]  (wl = w0 + lane)
// (G <= GR: a ring declared for the widest strip also serves the narrower ones; the unused slots are never allocated)
template <int G, int D, int GR>
__device__ __forceinline__ void wring_prime(WRing<GR, D>& R, const u32x4* __restrict__ wl, int wstride, int nk) {
    static_assert(G <= GR, "ring too narrow");
    // unconditional (a stream shorter than the ring re-loads its last k-step): the number of loads in flight stays a
    // compile-time constant, which is what lets the compiler's s_waitcnt placement be exact instead of draining the ring
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const int t = d < nk ? d : nk - 1;
#pragma unroll
        for (int g = 0; g < G; ++g) R.w[d][g] = wl[(int64_t)g * wstride + t * 64];
    }
}

// acc[i][g] += W(g, t0 + t) x X(i, t) for t < n, on a ring that holds k-steps t0 .. t0 + D - 1 (t0 % D == 0); refills the
// ring up to k-step nk_total.  xl -> LDS block layout (CBx column blocks per row block) of k-block t0.  The x fragments
// are double-buffered one k-step ahead (LDS latency only).
template <int G, int MB, int D, int XBP = -1, int GR>
__device__ __forceinline__ void mma_ring(WRing<GR, D>& R, const u32x4* __restrict__ wl, int wstride, int t0, int n, int nk_total,
                                         const char* xl, int CBx, int lane, f32x4 (&acc)[MB][G]) {
    static_assert(D % 2 == 0, "x double buffer follows the parity of the ring slot");
    // x fragments one k-step ahead only where registers allow (tiles of <= 2 row blocks; the 4-row-block update tiles run
    // 4 waves per SIMD, which covers the LDS latency) unless the caller says otherwise
    constexpr bool XB = XBP < 0 ? (MB <= 2) : (XBP != 0);
    const int r = lane & 15, q = lane >> 4;
    const char* xb = xl + (q >> 1) * 512 + r * 32 + (q & 1) * 16;
    u32x4 xa[MB], xc[XB ? MB : 1];
    if (XB) {
#pragma unroll
        for (int i = 0; i < MB; ++i) xa[i] = *reinterpret_cast<const u32x4*>(xb + (i * CBx) * 512);
    }
    // sched_barrier pins the order "x of the next k-step, MFMAs of this one, refill of this slot": left alone, the scheduler
    // sinks every load to just before its first use (fewer live registers) and the loop serialises on memory.
    for (int tt = 0; tt < n; tt += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int t = tt + d;
            if (t < n) {
                if (XB) {
                    if (t + 1 < n) {
#pragma unroll
                        for (int i = 0; i < MB; ++i) {
                            const u32x4 v = *reinterpret_cast<const u32x4*>(xb + (i * CBx + 2 * (t + 1)) * 512);
                            if (d & 1) xa[i] = v; else xc[i] = v;
                        }
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < MB; ++i) xa[i] = *reinterpret_cast<const u32x4*>(xb + (i * CBx + 2 * t) * 512);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < MB; ++i)
#pragma unroll
                    for (int g = 0; g < G; ++g) mma_frag<__bf16>(R.w[d][g], (XB && (d & 1)) ? xc[i] : xa[i], acc[i][g]);
                __builtin_amdgcn_sched_barrier(0);
                if (t0 + t + D < nk_total) {
#pragma unroll
                    for (int g = 0; g < G; ++g) R.w[d][g] = wl[(int64_t)g * wstride + (t0 + t + D) * 64];
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
}

// The two branch-free forms of the above.  Every k-step of the steady state issues the same loads in the same order, so the
// vmcnt the compiler derives for "slot d is ready" is the exact (D - 1) * G (+ whatever else is in flight); conditions
// around the refills (as in mma_ring) make its path-merging analysis assume the worst and drain the ring every revolution.
//
// mma_stream: a whole stream of nk k-steps (nk % D == 0, nk >= D) whose input is resident in LDS; ring primed with 0..D-1.
template <int G, int MB, int D, int XBP = -1, int GR>
__device__ __forceinline__ void mma_stream(WRing<GR, D>& R, const u32x4* __restrict__ wl, int wstride, int nk, const char* xl, int CBx,
                                           int lane, f32x4 (&acc)[MB][G]) {
    static_assert(D % 2 == 0, "x double buffer follows the parity of the ring slot");
    constexpr bool XB = XBP < 0 ? (MB <= 2) : (XBP != 0);
    const int r = lane & 15, q = lane >> 4;
    const char* xb = xl + (q >> 1) * 512 + r * 32 + (q & 1) * 16;
    u32x4 xa[MB], xc[XB ? MB : 1];
    if (XB) {
#pragma unroll
        for (int i = 0; i < MB; ++i) xa[i] = *reinterpret_cast<const u32x4*>(xb + (i * CBx) * 512);
    }
    int tt = 0;
    for (; tt + D < nk; tt += D) {          // steady state: refill every slot
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int t = tt + d;
            if (XB) {
#pragma unroll
                for (int i = 0; i < MB; ++i) {
                    const u32x4 v = *reinterpret_cast<const u32x4*>(xb + (i * CBx + 2 * (t + 1)) * 512);
                    if (d & 1) xa[i] = v; else xc[i] = v;
                }
            } else {
#pragma unroll
                for (int i = 0; i < MB; ++i) xa[i] = *reinterpret_cast<const u32x4*>(xb + (i * CBx + 2 * t) * 512);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < MB; ++i)
#pragma unroll
                for (int g = 0; g < G; ++g) mma_frag<__bf16>(R.w[d][g], (XB && (d & 1)) ? xc[i] : xa[i], acc[i][g]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = 0; g < G; ++g) R.w[d][g] = wl[(int64_t)g * wstride + (t + D) * 64];
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {           // last revolution: no refills
        const int t = tt + d;
        if (XB) {
            if (d + 1 < D) {
#pragma unroll
                for (int i = 0; i < MB; ++i) {
                    const u32x4 v = *reinterpret_cast<const u32x4*>(xb + (i * CBx + 2 * (t + 1)) * 512);
                    if (d & 1) xa[i] = v; else xc[i] = v;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < MB; ++i) xa[i] = *reinterpret_cast<const u32x4*>(xb + (i * CBx + 2 * t) * 512);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int g = 0; g < G; ++g) mma_frag<__bf16>(R.w[d][g], (XB && (d & 1)) ? xc[i] : xa[i], acc[i][g]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// mma_chunk: the 4 k-steps t0 .. t0 + 3 (t0 % 4 == 0, D divides 4) of a stream whose input arrives in 4-k-block LDS chunks
// (first layer); every slot is refilled, so at least one more chunk follows.  mma_chunk_last is the final chunk.
template <int G, int MB, int D, int XBP = -1, int GR>
__device__ __forceinline__ void mma_chunk(WRing<GR, D>& R, const u32x4* __restrict__ wl, int wstride, int t0, const char* xl, int CBx,
                                          int lane, f32x4 (&acc)[MB][G]) {
    static_assert(D == 2 || D == 4, "ring depth must divide the chunk");
    constexpr bool XB = XBP < 0 ? (MB <= 2) : (XBP != 0);
    const int r = lane & 15, q = lane >> 4;
    const char* xb = xl + (q >> 1) * 512 + r * 32 + (q & 1) * 16;
    u32x4 xa[MB], xc[XB ? MB : 1];
    if (XB) {
#pragma unroll
        for (int i = 0; i < MB; ++i) xa[i] = *reinterpret_cast<const u32x4*>(xb + (i * CBx) * 512);
    }
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
        const int d = s4 % D;
        if (XB) {
            if (s4 + 1 < 4) {
#pragma unroll
                for (int i = 0; i < MB; ++i) {
                    const u32x4 v = *reinterpret_cast<const u32x4*>(xb + (i * CBx + 2 * (s4 + 1)) * 512);
                    if (s4 & 1) xa[i] = v; else xc[i] = v;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < MB; ++i) xa[i] = *reinterpret_cast<const u32x4*>(xb + (i * CBx + 2 * s4) * 512);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int g = 0; g < G; ++g) mma_frag<__bf16>(R.w[d][g], (XB && (s4 & 1)) ? xc[i] : xa[i], acc[i][g]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < G; ++g) R.w[d][g] = wl[(int64_t)g * wstride + (t0 + s4 + D) * 64];
        __builtin_amdgcn_sched_barrier(0);
    }
}

// mma_chunk_n: a final chunk of exactly NL k-steps (1..4), straight-line: nothing beyond k-step t0 + NL - 1 is loaded.
template <int G, int MB, int D, int NL, int XBP = -1, int GR>
__device__ __forceinline__ void mma_chunk_n(WRing<GR, D>& R, const u32x4* __restrict__ wl, int wstride, int t0, const char* xl, int CBx,
                                            int lane, f32x4 (&acc)[MB][G]) {
    static_assert(NL >= 1 && NL <= 4 && (D == 2 || D == 4), "a chunk is 4 k-steps, the ring depth divides it");
    constexpr bool XB = XBP < 0 ? (MB <= 2) : (XBP != 0);
    const int r = lane & 15, q = lane >> 4;
    const char* xb = xl + (q >> 1) * 512 + r * 32 + (q & 1) * 16;
    u32x4 xa[MB], xc[XB ? MB : 1];
    if (XB) {
#pragma unroll
        for (int i = 0; i < MB; ++i) xa[i] = *reinterpret_cast<const u32x4*>(xb + (i * CBx) * 512);
    }
#pragma unroll
    for (int s4 = 0; s4 < NL; ++s4) {
        const int d = s4 % D;
        if (XB) {
            if (s4 + 1 < NL) {
#pragma unroll
                for (int i = 0; i < MB; ++i) {
                    const u32x4 v = *reinterpret_cast<const u32x4*>(xb + (i * CBx + 2 * (s4 + 1)) * 512);
                    if (s4 & 1) xa[i] = v; else xc[i] = v;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < MB; ++i) xa[i] = *reinterpret_cast<const u32x4*>(xb + (i * CBx + 2 * s4) * 512);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int g = 0; g < G; ++g) mma_frag<__bf16>(R.w[d][g], (XB && (s4 & 1)) ? xc[i] : xa[i], acc[i][g]);
        __builtin_amdgcn_sched_barrier(0);
        if (s4 + D < NL) {
#pragma unroll
            for (int g = 0; g < G; ++g) R.w[d][g] = wl[(int64_t)g * wstride + (t0 + s4 + D) * 64];
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// mma_chunk_last: the final chunk of a first layer -- its first nlast k-steps (1..4, wave-uniform; struct L0KSteps), the ones that
// hold a valid input column; the ring holds k-steps t0 .. t0 + min(D, nlast) - 1 (mma_chunk's refills, or wring_prime with the
// true remaining count).  ONE unrolled body, so that a kernel that carries several tile bodies pays for no second copy
// (mlp_fb_kernel has ~1 KB left of the 128 KiB a kernel may have): the MFMAs of a k-step at or beyond nlast are skipped by a
// wave-uniform branch around them.  Such a branch holds no load, so the number of loads in flight is the same on both sides of it
// and the vmcnt in front of every k-step stays as exact as in mma_stream; the x fragments are read regardless (LDS holds the whole
// staged chunk, zero-filled pad columns included).  Ring of 4: the chunk is resident, nothing is refilled.  Ring of 2: k-steps
// t0 + 2 / t0 + 3 are refilled behind k-steps t0 / t0 + 1, and a refill inside an `if` would join two paths with different
// counts -- the wait behind the join is then for the worse of the two.  So
//   * [t0 + 2] is issued whatever nlast is: for nlast <= 2 a fragment nobody reads (it lies inside the padded buffer);
//   * [t0 + 3] belongs to nlast = 4 alone, which takes a branch of its own from there on: [t0 + 3] k2 k3 against k2 for nlast = 3,
//     the one k-step that exists twice.
// COPY = false leaves that second k2 out where it does not fit (the update tiles on fp32 rows, mlp_fb_kernel<false>: four bodies,
// 130 000 bytes before this chunk form) and puts [t0 + 3] into an `if`: still exact for nlast = 3, which has nothing in flight
// behind k-step t0 + 2 either way, while nlast = 4 waits for k-steps t0 + 2 AND t0 + 3 in front of k2.
template <int G, int MB, int D, int XBP = -1, bool COPY = true, int GR>
__device__ __forceinline__ void mma_chunk_last(WRing<GR, D>& R, const u32x4* __restrict__ wl, int wstride, int t0, int nlast, const char* xl,
                                               int CBx, int lane, f32x4 (&acc)[MB][G]) {
    static_assert(D == 2 || D == 4, "ring depth must divide the chunk");
    constexpr bool XB = XBP < 0 ? (MB <= 2) : (XBP != 0);
    const int r = lane & 15, q = lane >> 4;
    const char* xb = xl + (q >> 1) * 512 + r * 32 + (q & 1) * 16;
    u32x4 xa[MB], xc[XB ? MB : 1];
    if (XB) {
#pragma unroll
        for (int i = 0; i < MB; ++i) xa[i] = *reinterpret_cast<const u32x4*>(xb + (i * CBx) * 512);
    }
    auto xread = [&](auto s4c) __attribute__((always_inline)) {           // the x fragments k-step s4 reads (XB: those of s4 + 1)
        constexpr int s4 = decltype(s4c)::value;
        if (XB) {
            if (s4 + 1 < 4) {
#pragma unroll
                for (int i = 0; i < MB; ++i) {
                    const u32x4 v = *reinterpret_cast<const u32x4*>(xb + (i * CBx + 2 * (s4 + 1)) * 512);
                    if (s4 & 1) xa[i] = v; else xc[i] = v;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < MB; ++i) xa[i] = *reinterpret_cast<const u32x4*>(xb + (i * CBx + 2 * s4) * 512);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    auto mfmas = [&](auto s4c) __attribute__((always_inline)) {
        constexpr int s4 = decltype(s4c)::value, d = s4 % D;
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int g = 0; g < G; ++g) mma_frag<__bf16>(R.w[d][g], (XB && (s4 & 1)) ? xc[i] : xa[i], acc[i][g]);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto refill = [&](auto s4c) __attribute__((always_inline)) {          // slot s4 % D <- k-step t0 + s4 + D (ring of 2 only)
        if constexpr (D == 2) {
            constexpr int s4 = decltype(s4c)::value, d = s4 % D;
#pragma unroll
            for (int g = 0; g < G; ++g) R.w[d][g] = wl[(int64_t)g * wstride + (t0 + s4 + D) * 64];
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    using K0 = std::integral_constant<int, 0>;
    using K1 = std::integral_constant<int, 1>;
    using K2 = std::integral_constant<int, 2>;
    using K3 = std::integral_constant<int, 3>;
    xread(K0());
    mfmas(K0());
    refill(K0());
    xread(K1());
    if (nlast > 1) mfmas(K1());
    if constexpr (D == 2 && COPY) {
        if (nlast > 3) {
            refill(K1());
            xread(K2());
            mfmas(K2());
            xread(K3());
            mfmas(K3());
        } else if (nlast > 2) {
            xread(K2());
            mfmas(K2());
        }
    } else {
        if (nlast > 3) refill(K1());
        xread(K2());
        if (nlast > 2) mfmas(K2());
        xread(K3());
        if (nlast > 3) mfmas(K3());
    }
}

// ELU of the bf16 path: exp(z) as v_exp_f32(z * log2 e).  The libm expf the fp32 parity path keeps (elu_f) is ~15 VALU
// instructions per element (argument split, ldexp, two range selects) and the epilogues were VALU-bound on them; the result
// is rounded to bf16 (2^-8 relative) right after, against this form's <= 1e-6 relative error for |z| <= 18.
// HGYM_ELU_FAST=0 restores elu_f.
__device__ __forceinline__ float elu_bf(float z) {
    return z > 0.0f ? z : (__builtin_amdgcn_exp2f(z * 1.4426950408889634f) - 1.0f);
}

// ---- any resolved activation (HgymNetConfig.fused_activation) -------------------------------------------------------------------
// Every fused device function below takes one more template parameter, GA: false = ELU(1), today's expressions (elu_bf in the
// epilogues, y > 0 ? 1 : y + 1 in the dZ chain) untouched; true = whatever struct Act (hgym_gemm.hpp) holds, carried in FwdArgs::act.
//
// Forward, v = f(v) over a wave's accumulators: one branch on the (wave-uniform) kind around the unrolled element loops, as
// act_fwd_tile has.  LeakyReLU / ReLU: z > 0 ? z : alpha z.  ELU(alpha) / SELU, Tanh and Sigmoid share one form built on
// E = expm1(t) -- ONE v_exp_f32 and ONE v_rcp_f32 per element, in the style of elu_bf:
//     ELU      t = z    scale * (z > 0 ? z : alpha * E)
//     Tanh     t = 2z   E / (E + 2)                          (= 1 - 2 / (1 + e^2z), without its cancellation at small |z|)
//     Sigmoid  t = z    e^t / (E + 2)                        (= 1 / (1 + e^-z))
// with E = exp2(t log2 e) - 1, and t (1 + t / 2) where |t| < 2^-6: there exp2() - 1 cancels (absolute error 1.2e-7, the spacing of
// fp32 at 1) while the two-term series is within t^2 / 6 <= 4e-5 relative, so E holds ~1e-5 relative or better everywhere -- far below
// bf16's 2^-9, which is what lets a planted pre-activation of 1e-6 come out within one bf16 ulp.  The exponent is clamped at 120, so
// e^t stays finite and E / (E + 2) = e^t / (E + 2) = 1 exactly from there on; towards -inf exp2 gives 0 and the forms give
// -scale alpha, -1 and 0.  No infinity meets a zero: nothing here can produce a NaN from a finite z.
//
// f(0) != 0 (Sigmoid: 0.5).  Nothing in the fused kernels relies on f(0) = 0 for its zero padding:
//   * rows past M in a tile re-read row M - 1 (clamped addresses), so their activations are those of a real row, finite under every
//     kind; their head gradient dZ3 is written as zero (`valid`), hence every dZ of the chain is 0 * f' = 0 and dW = dZ^T X adds nothing;
//   * the zeroed older frames of a reset row and the first layer's K padding (705 -> 768, zero input columns against zero weight
//     fragments) are zeros in the INPUT of a product: they add 0 to a pre-activation, and f is applied to the complete sum + bias;
//   * hidden widths are multiples of 128 and the head has no activation: no padded column ever passes through f.
template <int G, int MB>
__device__ __forceinline__ void act_any_tile(f32x4 (&v)[MB][G], const Act& a) {
#define HG_FACT_LOOP(BODY)                                       \
    _Pragma("unroll") for (int i = 0; i < MB; ++i)               \
        _Pragma("unroll") for (int g = 0; g < G; ++g)            \
            _Pragma("unroll") for (int e = 0; e < 4; ++e) { BODY; }
    if (a.kind == HGYM_ACT_LEAKY_RELU) {
        const float al = a.alpha;
        HG_FACT_LOOP(const float z = v[i][g][e]; v[i][g][e] = z > 0.0f ? z : __builtin_fmaf(al, z, 0.0f))      /* (+ 0: ReLU's al z = -0 becomes the +0 that f gives) */
        return;
    }
    const bool elu = a.kind == HGYM_ACT_ELU, sig = a.kind == HGYM_ACT_SIGMOID;
    const float c2 = a.kind == HGYM_ACT_TANH ? 2.0f : 1.0f, k = c2 * 1.4426950408889634f;
    const float q = elu ? 0.0f : 1.0f, d0 = elu ? 1.0f : 2.0f;          // denominator q E + d0: 1 (ELU), E + 2
    const float sn = elu ? a.scale * a.alpha : 1.0f, sp = a.scale;
    const float thr = elu ? 0.0f : INFINITY;                            // the linear side exists for ELU only
    HG_FACT_LOOP(const float z = v[i][g][e]; const float t = z * c2;
                 const float ex = __builtin_amdgcn_exp2f(fminf(z * k, 120.0f));
                 const float em1 = fabsf(t) < 0.015625f ? t * __builtin_fmaf(0.5f, t, 1.0f) : ex - 1.0f;
                 const float y = (sn * (sig ? ex : em1)) * __builtin_amdgcn_rcpf(__builtin_fmaf(q, em1, d0));
                 v[i][g][e] = z > thr ? sp * z : y)
#undef HG_FACT_LOOP
}

// bias + ELU, bf16, -> LDS block layout (next layer's input) and, when Hg != null, the same blocks in HBM
// (GA: bias + FwdArgs::act, applied to the accumulators in place ahead of the stores)
template <int G, int MB, bool STORE, bool GA = false>
__device__ __forceinline__ void epilogue_elu_t(f32x4 (&acc)[MB][G], const float* __restrict__ bias, int nb0, char* out_lds, int CBo,
                                               __bf16* __restrict__ Hg, int64_t mbg0, int lane, const Act& fn) {
    const int r = lane & 15, q = lane >> 4;
    const int loff = r * 32 + q * 8;
    static_assert(MB % 2 == 0, "row blocks are stored in pairs");
    if constexpr (GA) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const F4 b = *reinterpret_cast<const F4*>(bias + (nb0 + g) * 16 + 4 * q);
#pragma unroll
            for (int i = 0; i < MB; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][g][e] += b.v[e];
        }
        act_any_tile<G, MB>(acc, fn);
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        F4 b = {{0.f, 0.f, 0.f, 0.f}};
        if constexpr (!GA) b = *reinterpret_cast<const F4*>(bias + (nb0 + g) * 16 + 4 * q);
#pragma unroll
        for (int i = 0; i < MB; i += 2) {
            u32x2 pk[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float v[4];
                if constexpr (GA) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc[i + h][g][e];
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = elu_bf(acc[i + h][g][e] + b.v[e]);
                }
                pk[h] = pack_bf16x4(v[0], v[1], v[2], v[3]);
                *reinterpret_cast<u32x2*>(out_lds + ((i + h) * CBo + nb0 + g) * 512 + loff) = pk[h];
            }
            if (STORE) {
                char* pa = reinterpret_cast<char*>(Hg) + ((mbg0 + i) * CBo + nb0 + g) * 512 + loff;
                st_pair<(kFusedNT & 2) != 0, false>(pa, pa + (int64_t)CBo * 512, pk[0], pk[1], true, true, q);
            }
        }
    }
}
// (the store decision is wave-uniform and taken once here, not per block inside the unrolled epilogue)
template <int G, int MB, bool GA = false>
__device__ __forceinline__ void epilogue_elu(f32x4 (&acc)[MB][G], const float* __restrict__ bias, int nb0, char* out_lds, int CBo,
                                             __bf16* __restrict__ Hg, int64_t mbg0, int lane, const Act& fn) {
    if (Hg) epilogue_elu_t<G, MB, true, GA>(acc, bias, nb0, out_lds, CBo, Hg, mbg0, lane, fn);
    else epilogue_elu_t<G, MB, false, GA>(acc, bias, nb0, out_lds, CBo, Hg, mbg0, lane, fn);
}

template <int G, int MB>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[MB][G]) {
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int g = 0; g < G; ++g) acc[i][g] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// one hidden layer whose whole input is resident in LDS: waves split the n-blocks, G per strip.  R holds the primed stream
// of this wave's first strip (hidden_prime).  With AHEAD (8-wave tiles: registers to spare) `prime_next` is called before the
// epilogue of the last strip, so the following layer's stream is in flight across the epilogue and the barrier; without it
// the caller primes after the barrier.
template <int G, int D, int GR>
__device__ __forceinline__ void hidden_prime(WRing<GR, D>& R, const FusedLayer& L, int wave, int lane) {
    const int nb0 = wave * G;
    if (nb0 < L.NB) wring_prime<G, D>(R, L.Wf + (int64_t)nb0 * L.KB * 64 + lane, L.KB * 64, L.KB);
}

template <int G, int MB, int NW, int D, bool AHEAD, bool GA = false, int GR, class Next>
__device__ __forceinline__ void hidden_layer(WRing<GR, D>& R, const FusedLayer& L, const float* bias, const char* in_lds, int CBin,
                                             char* out_lds, __bf16* Hg, int64_t mbg0, int wave, int lane, Next prime_next, const Act& fn) {
    bool primed = false;
    for (int nb0 = wave * G; nb0 < L.NB; nb0 += NW * G) {
        f32x4 acc[MB][G];
        zero_acc<G, MB>(acc);
        const u32x4* wl = L.Wf + (int64_t)nb0 * L.KB * 64 + lane;
        constexpr int XBF = NW <= 8 ? 1 : -1;
        if (L.KB % D == 0) mma_stream<G, MB, D, XBF>(R, wl, L.KB * 64, L.KB, in_lds, CBin, lane, acc);
        else mma_ring<G, MB, D, XBF>(R, wl, L.KB * 64, 0, L.KB, L.KB, in_lds, CBin, lane, acc);
        const int nxt = nb0 + NW * G;
        if (nxt < L.NB) wring_prime<G, D>(R, L.Wf + (int64_t)nxt * L.KB * 64 + lane, L.KB * 64, L.KB);
        else if (AHEAD) { prime_next(); primed = true; }
        epilogue_elu<G, MB, GA>(acc, bias, nb0, out_lds, L.NB, Hg, mbg0, lane, fn);
    }
    if (AHEAD && !primed) prime_next();       // waves without a strip in this layer
}

// optional phase timestamps (hgym_prof_phase_buffer): thread 0 of every workgroup writes the 100 MHz wall clock at phase
// boundaries into dbg[(blockIdx.y * gridDim.x + blockIdx.x) * 8 + slot]
__device__ __forceinline__ void phase_stamp(long long* dbg, int slot) {
    if (dbg && threadIdx.x == 0) dbg[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 8 + slot] = (long long)__builtin_amdgcn_s_memrealtime();
}

// log(sigma) of the sampling epilogue: hardware log2 times ln 2 as ONE non-fusable multiply.  libm's logf is inlined library
// code whose internal multiply-adds the backend contracts or not depending on the translation unit's -ffp-contract setting, so
// it returned different last bits in hgym_net.hip and hgym_rollout.hip; this form is the same instruction pair everywhere
// (<= 2 ulp of log for sigma in [1e-3, 1e3]; the log-probability is compared with the reference at 1e-5 relative).
__device__ __forceinline__ float log_sigma(float s) { return __fmul_rn(__builtin_amdgcn_logf(s), 0.6931471805599453f); }

// ---- the actor's first layer carried ACROSS launches of the rollout (round 4) ----------------------------------------------------
// An observation row is a stack of frames: the row of step t + 1 is the row of step t shifted by one frame (47 columns) plus the
// frame step t produces, so columns [0, 640) of the NEXT row -- 20 of the first layer's 24 k-steps -- are known when launch t starts.
// Launch t's critic workgroup of the tile (idle from ~16 us of the ~40 us launch on; in the 64-row layout of the steady-state launch
// the side-job workgroup of two tiles) forms those k-steps of the actor's first layer for the next row (`l0_partial_ahead`) and
// leaves the fp32 accumulators in the caller's scratch; launch t + 1's actor tile
// (`fwd_body<.., PART>`) starts from them and runs the last 128-column chunk only: the same fragments, the same k order, the same
// accumulator chain -- the pre-activations are bit-identical -- and 8 of the first layer's 9.5 us leave the launch's critical path.
// Rows whose env was reset in between have zero older frames: their partial sums are dropped (0 + the chunk's products, as the
// reference computes on a zero history).
struct L0Part {
    const float* acc;        // [tile][wave][MB * G1][64 lanes][4]: pre-activations over k-steps [0, kb0) left by the previous launch
    const uint8_t* reset;    // (M,) the previous step's reset flags
    int kb0;                 // first k-step still to do here (a multiple of 4: whole 128-column chunks)
};
struct L0Ahead {
    float* acc_out;          // the same layout, for the NEXT launch (null: nothing to do)
    __bf16* xs_next;         // bf16 shadow rows of the next step's observation: columns [0, 32 kb0) are written here (null: no shadow)
    int64_t ldxs;
    int shift;               // columns a row shifts by per step (one frame)
    int kb0;                 // k-steps formed ahead
};

// by ALL 8 wavefronts of a workgroup (the caller has synchronised if the workgroup ran a tile of its own before): rows
// tile * BM .. tile * BM + BM - 1 of net n's fp32 input, columns [shift, shift + 32 kb0) -> bf16 (the rounding fwd_body's staging
// applies) -> LDS block layout -> k-steps [0, kb0) of the first layer with fwd_body<32, 8, 4, G1>'s wave -> strip mapping -> acc_out,
// in the layout of the 32-row actor tiles that consume it (a 64-row call streams the weights once for two of them).  kb0 % 4 == 0.
template <int G1, int BM = 32>
__device__ __forceinline__ void l0_partial_ahead(const FusedNet& n, const L0Ahead& ah, int M, char* smem, int tile) {
    static_assert(BM == 32 || BM == 64, "whole 32-row actor tiles");
    constexpr int NW = 8, MB = BM / 16, D = 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = tile * BM;
    const FusedLayer& L0 = n.layer[0];
    const int CB = 2 * ah.kb0, groups = 8 * ah.kb0;          // column blocks of 16 / groups of 4 columns per row
    const int nb0 = wave * G1;
    WRing<G1, D> r0;
    const u32x4* wl0 = L0.Wf + (int64_t)nb0 * L0.KB * 64 + lane;
    wring_prime<G1, D>(r0, wl0, L0.KB * 64, ah.kb0);
    constexpr int IPR = 5 * BM / 32;                             // items per lane per round: (row, 4 consecutive new columns)
    for (int j0 = 0; j0 < BM * groups; j0 += NW * 64 * IPR) {
        F4 v[IPR];
        int row[IPR], c4[IPR];
#pragma unroll
        for (int u = 0; u < IPR; ++u) {
            int j = j0 + u * NW * 64 + tid;
            j = j < BM * groups ? j : BM * groups - 1;
            row[u] = j / groups;
            c4[u] = (j - row[u] * groups) * 4;
            int m = m0 + row[u];
            m = m < M ? m : M - 1;
            v[u] = *reinterpret_cast<const F4*>(n.x + (int64_t)m * n.ldx + ah.shift + c4[u]);
        }
#pragma unroll
        for (int u = 0; u < IPR; ++u) {
            const u32x2 pk = pack_bf16x4(v[u].v[0], v[u].v[1], v[u].v[2], v[u].v[3]);
            *reinterpret_cast<u32x2*>(smem + ((row[u] >> 4) * CB + (c4[u] >> 4)) * 512 + (row[u] & 15) * 32 + ((c4[u] >> 2) & 3) * 8) = pk;
            if (ah.xs_next && m0 + row[u] < M && j0 + u * NW * 64 + tid < BM * groups)
                st_stream_u2<(kFusedNT & 2) != 0>(reinterpret_cast<char*>(ah.xs_next + (int64_t)(m0 + row[u]) * ah.ldxs + c4[u]), pk);
        }
    }
    __syncthreads();
    f32x4 acc[MB][G1];
    zero_acc<G1, MB>(acc);
    mma_stream<G1, MB, D, 1>(r0, wl0, L0.KB * 64, ah.kb0, smem, CB, lane, acc);
    // row block i belongs to 32-row tile tile * BM / 32 + i / 2, where it is that tile's row block i % 2
#pragma unroll
    for (int i = 0; i < MB; ++i) {
        f32x4* dst = reinterpret_cast<f32x4*>(ah.acc_out) + ((int64_t)((tile * (BM / 32) + i / 2) * NW + wave) * (2 * G1) + (i & 1) * G1) * 64 + lane;
#pragma unroll
        for (int g = 0; g < G1; ++g) dst[g * 64] = acc[i][g];
    }
}

struct FwdArgs {
    long long* dbg;
    FusedNet net[3];           // 0 actor, 1 critic, 2 auxiliary head
    int net0;                 // net index of blockIdx.y == 0
    int M;
    const int64_t* idx;       // optional row gather
    int train;                // write X0 / H[] for the backward pass
    int sample;               // actor head epilogue: Gaussian sample + log-prob (PPO.act)
    int A;                    // num_actions
    const float* std_;        // [A]
    const float* z;           // optional (M, A) normals; null -> Philox(k0, k1, *step)
    uint32_t k0, k1;
    const int64_t* step;
    float* actions;           // (M, A)
    float* sigma;             // (M, A)
    float* logp;              // (M,)
    int nets;                 // networks in this launch (blockIdx.y < nets)
    FinArgs fin;              // postponed env-step finaliser riding in this launch (blockIdx.y == nets, one workgroup); fin.N == 0: none
    Act act;                  // the hidden layers' activation of every net of the launch; read by the GA instantiations only (last member:
                              // no other member's offset in the kernel argument moves)
};

// Hooks of the fused rollout step (hgym_rollout.hip), three callables: `early()` runs once per workgroup right after the tile's
// first loads (bias, first weight k-steps, first input chunk) have been ISSUED and before anything waits for them -- the env
// step's own input loads and its Philox draws go there, under the same memory round trip; `mid()` runs between the first
// layer and the second, where the first layer's weight ring and accumulators are dead and ~60 registers are free for loads that
// may take the rest of the tile to arrive (the observation history); `put_action(row, j, a)` receives every sampled action of
// the tile (row within the tile, action index) so that the env phase reads them from LDS; `idle()` runs on the wavefronts that
// have no head block while the others compute the head; `head(wave, row, nb, out[4])` runs on the head wavefronts with each lane's
// row, the head's 16-column block and its four head outputs (the fused forward + backward kernel computes the PPO loss gradient there).  They are lambdas that capture the
// caller's locals by reference (a hook OBJECT carrying the prefetch arrays as members was kept in private memory by the
// compiler: 500 scratch instructions and a kernel four times slower).
// `extra` (whatever the hooks need from the kernel argument) reaches them as a call PARAMETER: a closure that captured a
// reference to the kernel argument would count as a capture of the whole argument block, of which the compiler then keeps a
// private-memory copy (3 KB of scratch per lane).
struct FwdNoop {
    template <class X> __device__ __forceinline__ void operator()(const X&) const {}
    __device__ __forceinline__ void operator()(int, int, float) const {}
    __device__ __forceinline__ void operator()(int, int, int, const float (&)[4]) const {}
};

template <int BM, int NW, int D, int G1, bool WIDE = false, bool XB16 = false, bool PART = false, bool GA = false, class Early = FwdNoop, class Mid = FwdNoop,
          class Put = FwdNoop, class Extra = int, class Idle = FwdNoop, class Head = FwdNoop, class L2Idle = FwdNoop>
__device__ __forceinline__ void fwd_body(const FwdArgs& a, const FusedNet& n, bool is_actor, char* smem, Early&& hook_early = Early(),
                                         Mid&& hook_mid = Mid(), Put&& hook_put = Put(), const Extra& extra = Extra(),
                                         Idle&& hook_idle = Idle(), Head&& hook_head = Head(), char* h2_lds = nullptr,
                                         int* rowidx_lds = nullptr, L2Idle&& hook_l2idle = L2Idle(), const L0Part* part = nullptr,
                                         int tile = -1) {
    // PART (the rollout's actor tile, hgym_rollout.hip): the first layer starts from the partial sums *part and runs chunks
    // [part->kb0 / 4, NC) only (struct L0Part above)
    static_assert(!PART || !XB16, "the carried first layer exists for fp32 input rows only");
    // rowidx_lds (BM ints of LDS): receives the storage row of every tile row (a.idx gathered once, by the lanes that stage the
    // input) for whoever needs it later in the tile; hook_l2idle(extra): runs on the wavefronts that have no strip in the third
    // layer while the others compute it (the fused forward + backward kernel gathers its loss inputs there).
    // tile: the BM-row tile this workgroup computes (-1: blockIdx.x; the rollout's 64-row critic tiles sit at other grid columns)
    constexpr int MB = BM / 16;
    constexpr int IT = BM * 32 / (NW * 64);           // staging items per thread per chunk (BM rows x 32 float4)
    constexpr int RPP = NW * 2;                       // rows covered per staging pass (32 lanes per row)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int m0 = (tile < 0 ? (int)blockIdx.x : tile) * BM;
    const int64_t mbg0 = m0 >> 4;
    char* P = smem;
    char* Q = smem + fused_lds_p(n, BM);
    // third-layer activations: over the first layer's (dead) in P, unless the caller wants H0 to survive (the fused forward +
    // backward kernel needs all three for its dZ chain) and provides a buffer of BM x layer[2].N bf16
    char* PH2 = h2_lds ? h2_lds : P;
    const FusedLayer& L0 = n.layer[0];
    const FusedLayer& L1 = n.layer[1];
    const FusedLayer& L2 = n.layer[2];
    const FusedLayer& L3 = n.layer[3];
    const int train = (a.train & 1) && n.X0, train_h = a.train & 2;     // bit 0: write X0 (a net without an X0 buffer shares another net's copy of the same rows), bit 1: write H[]
    // the four bias vectors -> LDS: the loads are issued here, ahead of everything else, and parked in registers; they are
    // written to LDS next to the first input chunk, so no epilogue ever waits on a cold global load
    float* bl = reinterpret_cast<float*>(smem + fused_lds_p(n, BM) + fused_lds_q(n, BM));
    constexpr int BIT = (768 + 768 + 768 + 96 + NW * 64 - 1) / (NW * 64);     // fused_supported: hidden widths <= 768, head <= 96
    float bv[BIT];
    const int bn0 = L0.N, bn1 = bn0 + L1.N, bn2 = bn1 + L2.N, bn3 = bn2 + (WIDE ? 16 * L3.NB : 16);
#pragma unroll
    for (int u = 0; u < BIT; ++u) {
        int i = tid + u * NW * 64;
        i = i < bn2 + L3.N ? i : bn2 + L3.N - 1;          // clamp: the pad entries re-read the last head bias (never used)
        const float* src = i < bn0 ? L0.bias + i : (i < bn1 ? L1.bias + (i - bn0) : (i < bn2 ? L2.bias + (i - bn1) : L3.bias + (i - bn2)));
        bv[u] = *src;
    }
    // sampling epilogue inputs (head waves of the actor): fetched now, used ~20 us later
    constexpr bool HOIST = NW <= 8;      // the 16-wave tiles have no registers to park them in (they spill)
    int64_t step_pre = 0;
    float std_pre[4] = {1.0f, 1.0f, 1.0f, 1.0f}, lsg_pre[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (HOIST && is_actor && a.sample && wave < BM / 16) {
        if (!a.z && a.step) step_pre = a.step[0];
#pragma unroll
        for (int e = 0; e < 4; ++e) std_pre[e] = a.std_[4 * q + e < a.A ? 4 * q + e : 0];
#pragma unroll
        for (int e = 0; e < 4; ++e) lsg_pre[e] = log_sigma(std_pre[e]);      // under the first input load instead of in the tail
    }
    auto bias_to_lds = [&]() {
#pragma unroll
        for (int u = 0; u < BIT; ++u) {
            const int i = tid + u * NW * 64;
            if (i < bn3) bl[i] = bv[u];
        }
    };
    constexpr bool AHEAD = NW <= 8;
    constexpr int XBF = NW <= 8 ? 1 : -1;  // 8-wave tiles have the registers to keep the x fragments one k-step ahead
    constexpr int GH = NW <= 8 ? 2 : 1;   // n-blocks per strip in the hidden layers (widths are multiples of 128 = 8 n-blocks)
    WRing<GH, D> r1, r2;             // weight streams of the two hidden layers
    auto prime1 = [&]() { hidden_prime<GH, D>(r1, L1, wave, lane); };

    // ---------------------------------------------------------------- layer 0: input streamed in 128-column chunks
    // k-steps the loop runs (struct L0KSteps).  The 64-row tile on 8 wavefronts (the rollout launch's critic tile: 6 n-blocks a wave,
    // 254 VGPRs in a kernel that has no scratch) keeps all KB of them in the straight-line form: either short form costs it spills.
    constexpr bool L0_FULL = NW <= 8 && D == 2;
    const int KR0 = (!L0_FULL && HGYM_L0_TRIM >= (D == 4 ? 1 : 2)) ? L0.KR : L0.KB;
    if constexpr (XB16) {
        // input rows from the bf16 shadow: a chunk is 64 (32) rows x 256 B = one 16-byte item per lane, loaded as it will lie in
        // LDS.  Lane map: 16 consecutive lanes = 8 rows x the two halves of one block row (a conflict-free 256-byte LDS
        // write), the four lane groups = four consecutive column blocks (128 contiguous bytes of each row per instruction);
        // waves = row groups of 8 x the two halves of the chunk.
        constexpr int RG = BM / 8;
        static_assert(NW == 2 * RG, "one 16-byte item per lane per chunk");
        const int NC = L0.KB / 4;
        const int row = (wave % RG) * 8 + ((lane >> 1) & 7), cb = (wave / RG) * 4 + (lane >> 4), hf = lane & 1;
        int m = m0 + row;
        m = m < a.M ? m : a.M - 1;
        const int64_t src = a.idx ? a.idx[m] : (int64_t)m;
        const char* srow = reinterpret_cast<const char*>(n.xb + src * n.ldxb + cb * 16 + hf * 8);
        if (rowidx_lds && cb == 0 && hf == 0) rowidx_lds[row] = (int)src;
        const int loff = ((row >> 4) * 8 + cb) * 512 + (row & 15) * 32 + hf * 16;
        u32x4 stg;
        auto stage_load = [&](int c) { stg = ld_stream_u4<(kFusedNT & 1) != 0>(srow + c * (FUSED_CHUNK * 2)); };
        auto stage_write = [&](int buf) { *reinterpret_cast<u32x4*>(Q + buf * (BM * FUSED_CHUNK * 2) + loff) = stg; };
        const int nb0 = wave * G1;
        f32x4 acc[MB][G1];
        zero_acc<G1, MB>(acc);
        WRing<G1, D> r0;
        const u32x4* wl0 = L0.Wf + (int64_t)nb0 * L0.KB * 64 + lane;
        phase_stamp(a.dbg, 0);
        wring_prime<G1, D>(r0, wl0, L0.KB * 64, KR0);
        stage_load(0);
        hook_early(extra);
        stage_write(0);
        bias_to_lds();
        __syncthreads();
        phase_stamp(a.dbg, 1);
        // (the staging keeps whole chunks: the pad columns it copies are the zeros the shadow holds)
        for (int c = 0; c + 1 < NC; ++c) {
            stage_load(c + 1);
            mma_chunk<G1, MB, D, XBF>(r0, wl0, L0.KB * 64, c * 4, Q + (c & 1) * (BM * FUSED_CHUNK * 2), 8, lane, acc);
            stage_write((c + 1) & 1);
            __syncthreads();
        }
        mma_chunk_last<G1, MB, D, XBF>(r0, wl0, L0.KB * 64, (NC - 1) * 4, KR0 - (NC - 1) * 4, Q + ((NC - 1) & 1) * (BM * FUSED_CHUNK * 2), 8, lane, acc);
        phase_stamp(a.dbg, 2);
        if (AHEAD) prime1();
        epilogue_elu<G1, MB, GA>(acc, bl, nb0, P, L0.NB, train_h ? n.H[0] : nullptr, mbg0, lane, a.act);
    } else {
        const int NC = L0.KB / 4;
        const int CB0 = 2 * L0.KB;
        const int f4 = tid & 31;
        const float* srow[IT];
        int lrow[IT];
#pragma unroll
        for (int u = 0; u < IT; ++u) {
            const int row = u * RPP + (tid >> 5);
            int m = m0 + row;
            m = m < a.M ? m : a.M - 1;
            const int64_t src = a.idx ? a.idx[m] : (int64_t)m;
            srow[u] = n.x + src * n.ldx;
            lrow[u] = row;
            if (rowidx_lds && f4 == 0) rowidx_lds[row] = (int)src;
        }
        F4 stg[IT];
        // one unconditional 16-byte load per item: the address is clamped to the last full vector of the row.  stage_load
        // ONLY issues the loads (nothing here may consume them: the data must stay in flight under the MFMAs of the current
        // chunk); stage_write re-aligns / zero-fills the (at most one per row) straddling item with selects, converts and
        // stores to LDS.
        auto stage_load = [&](int c) {
            const int col = c * FUSED_CHUNK + f4 * 4;
            const int cc = col < L0.K - 4 ? col : L0.K - 4;
#pragma unroll
            for (int u = 0; u < IT; ++u) stg[u] = ld_stream_f4<(kFusedNT & 1) != 0>(srow[u] + cc);
        };
        auto stage_write = [&](int c, int buf) {
            char* dst = Q + buf * (BM * FUSED_CHUNK * 2);
            const int col = c * FUSED_CHUNK + f4 * 4;
            const int cc = col < L0.K - 4 ? col : L0.K - 4;
            const int sh = col - cc;                       // 0 for full items, 1..3 for the straddling one, >= 4: all padding
#pragma unroll
            for (int u = 0; u < IT; ++u) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = e + sh;
                    float r = 0.0f;
                    r = k == 0 ? stg[u].v[0] : r;
                    r = k == 1 ? stg[u].v[1] : r;
                    r = k == 2 ? stg[u].v[2] : r;
                    r = k == 3 ? stg[u].v[3] : r;
                    v[e] = r;
                }
                const u32x2 pk = pack_bf16x4(v[0], v[1], v[2], v[3]);
                const int inblk = (lrow[u] & 15) * 32 + (f4 & 3) * 8;
                *reinterpret_cast<u32x2*>(dst + ((lrow[u] >> 4) * 8 + (f4 >> 2)) * 512 + inblk) = pk;
                if (train)
                    st_stream_u2<(kFusedNT & 2) != 0>(reinterpret_cast<char*>(n.X0) +
                                                     ((mbg0 + (lrow[u] >> 4)) * CB0 + c * 8 + (f4 >> 2)) * 512 + inblk, pk);
                if (n.xs && m0 + lrow[u] < a.M)      // row m of the bf16 shadow (pad columns receive the zeros formed above)
                    st_stream_u2<(kFusedNT & 2) != 0>(reinterpret_cast<char*>(n.xs + (int64_t)(m0 + lrow[u]) * n.ldxs + col), pk);
            }
        };
        const int nb0 = wave * G1;
        f32x4 acc[MB][G1];
        const int c0 = PART ? part->kb0 / 4 : 0;                // first chunk this launch runs; k-steps and LDS buffers count from it
        bool drop[MB];
        if constexpr (PART) {
            const f32x4* src = reinterpret_cast<const f32x4*>(part->acc) + ((int64_t)(blockIdx.x * NW + wave) * (MB * G1)) * 64 + lane;
#pragma unroll
            for (int i = 0; i < MB; ++i)
#pragma unroll
                for (int g = 0; g < G1; ++g) acc[i][g] = src[(i * G1 + g) * 64];
#pragma unroll
            for (int i = 0; i < MB; ++i) {                      // lane (r, q) holds row i * 16 + r of the tile
                int m = m0 + i * 16 + r;
                m = m < a.M ? m : a.M - 1;
                drop[i] = part->reset[m] != 0;
            }
        } else {
            zero_acc<G1, MB>(acc);
        }
        WRing<G1, D> r0;
        const u32x4* wl0 = L0.Wf + (int64_t)nb0 * L0.KB * 64 + lane + (int64_t)c0 * 4 * 64;
        phase_stamp(a.dbg, 0);
        wring_prime<G1, D>(r0, wl0, L0.KB * 64, KR0 - c0 * 4);
        stage_load(c0);
        hook_early(extra);
        stage_write(c0, 0);
        bias_to_lds();
        if constexpr (PART) {
#pragma unroll
            for (int i = 0; i < MB; ++i)
#pragma unroll
                for (int g = 0; g < G1; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[i][g][e] = drop[i] ? 0.0f : acc[i][g][e];
        }
        __syncthreads();
        phase_stamp(a.dbg, 1);
        // steady state: no condition inside the body (see mma_stream); the last chunk is peeled
        for (int c = c0; c + 1 < NC; ++c) {
            stage_load(c + 1);
            mma_chunk<G1, MB, D, XBF>(r0, wl0, L0.KB * 64, (c - c0) * 4, Q + ((c - c0) & 1) * (BM * FUSED_CHUNK * 2), 8, lane, acc);
            stage_write(c + 1, (c + 1 - c0) & 1);
            __syncthreads();
        }
        // (the staging keeps whole chunks: the zero-filled pad columns still reach LDS, the shadow and X0)
        if constexpr (L0_FULL) mma_chunk_n<G1, MB, D, 4, XBF>(r0, wl0, L0.KB * 64, (NC - 1 - c0) * 4, Q + ((NC - 1 - c0) & 1) * (BM * FUSED_CHUNK * 2), 8, lane, acc);
        else mma_chunk_last<G1, MB, D, XBF, NW <= 8>(r0, wl0, L0.KB * 64, (NC - 1 - c0) * 4, KR0 - (NC - 1) * 4, Q + ((NC - 1 - c0) & 1) * (BM * FUSED_CHUNK * 2), 8, lane, acc);
        phase_stamp(a.dbg, 2);
        if (AHEAD) prime1();
        epilogue_elu<G1, MB, GA>(acc, bl, nb0, P, L0.NB, train_h ? n.H[0] : nullptr, mbg0, lane, a.act);
    }
    __syncthreads();
    phase_stamp(a.dbg, 3);
    hook_mid(extra);
    if (!AHEAD) prime1();
    // ---------------------------------------------------------------- layers 1, 2: input resident in LDS
    auto prime2 = [&]() { hidden_prime<GH, D>(r2, L2, wave, lane); };
    hidden_layer<GH, MB, NW, D, AHEAD, GA>(r1, L1, bl + L0.N, P, L0.NB, Q, train_h ? n.H[1] : nullptr, mbg0, wave, lane, prime2, a.act);
    __syncthreads();
    phase_stamp(a.dbg, 4);
    if (!AHEAD) prime2();
    WRing<1, 4> r3;                  // head: one 16-row block per wave, L3.KB k-steps of one fragment
    auto prime3 = [&]() {
        if (wave < MB) wring_prime<1, 4>(r3, L3.Wf + lane, 0, L3.KB);
    };
    hidden_layer<GH, MB, NW, D, AHEAD, GA>(r2, L2, bl + L0.N + L1.N, Q, L1.NB, PH2, train_h ? n.H[2] : nullptr, mbg0, wave, lane, prime3, a.act);
    if (wave * GH >= L2.NB) hook_l2idle(extra);       // wavefronts without a strip in this layer
    __syncthreads();
    phase_stamp(a.dbg, 5);
    if (!AHEAD) prime3();
    // ---------------------------------------------------------------- head: one wave per 16-row block
    if (wave < MB) {
        f32x4 hacc[1][1];
        hacc[0][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const int CB3 = L2.NB;
        if (L3.KB % 4 == 0) mma_stream<1, 1, 4>(r3, L3.Wf + lane, 0, L3.KB, PH2 + wave * CB3 * 512, CB3, lane, hacc);
        else mma_ring<1, 1, 4>(r3, L3.Wf + lane, 0, 0, L3.KB, L3.KB, PH2 + wave * CB3 * 512, CB3, lane, hacc);
        const f32x4 acc = hacc[0][0];
        const int m = m0 + wave * 16 + r;
        const int No = L3.N;
        float mu[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) mu[e] = acc[e] + ((4 * q + e < No) ? bl[L0.N + L1.N + L2.N + 4 * q + e] : 0.0f);
        if (m < a.M && n.out) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * q + e < No) n.out[(int64_t)m * n.ldo + 4 * q + e] = mu[e];
        }
        hook_head(wave, m, 0, mu);  // `idle()`'s counterpart: every lane of the head wavefronts, with its row, the head's column block and its 4 outputs
        if (is_actor && a.sample) {
#pragma clang fp contract(off)      // a = mu + sigma z and the log-probability as separate fp32 roundings, identically in every translation unit
            const int A = a.A;
            float zz[4];
            if (a.z) {
#pragma unroll
                for (int e = 0; e < 4; ++e) zz[e] = (m < a.M && 4 * q + e < A) ? a.z[(int64_t)m * A + 4 * q + e] : 0.0f;
            } else {
                const int64_t s = HOIST ? step_pre : (a.step ? a.step[0] : 0);
                const RngKey rk = {a.k0, a.k1, (uint32_t)s, (uint32_t)(s >> 32)};
                const U4 u = rng4(rk, (uint32_t)m, SLOT_POLICY + (uint32_t)q);
                box_muller(u.x, u.y, zz[0], zz[1]);
                box_muller(u.z, u.w, zz[2], zz[3]);
            }
            float lp = 0.0f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = 4 * q + e;
                if (j < A) {
                    const float sg = mu[e] * 0.0f + (HOIST ? std_pre[e] : a.std_[j]);      // actor_critic.py:113
                    const float act = mu[e] + sg * zz[e];
                    const float d = act - mu[e];
                    lp += -(d * d) / (2.0f * sg * sg) - (HOIST ? lsg_pre[e] : log_sigma(sg)) - 0.9189385332046727f;
                    if (m < a.M) {
                        a.actions[(int64_t)m * A + j] = act;
                        a.sigma[(int64_t)m * A + j] = sg;
                    }
                    hook_put(wave * 16 + r, j, act);
                }
            }
            lp += __shfl_xor(lp, 16, 64);
            lp += __shfl_xor(lp, 32, 64);
            if (q == 0 && m < a.M) a.logp[m] = lp;
        }
        // heads wider than one n-block (the auxiliary net, its own instantiation): the remaining blocks, same wave, one after
        // the other
        for (int nb = 1; WIDE && nb < L3.NB; ++nb) {
            const u32x4* wl = L3.Wf + (int64_t)nb * L3.KB * 64 + lane;
            wring_prime<1, 4>(r3, wl, 0, L3.KB);
            hacc[0][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (L3.KB % 4 == 0) mma_stream<1, 1, 4>(r3, wl, 0, L3.KB, PH2 + wave * CB3 * 512, CB3, lane, hacc);
            else mma_ring<1, 1, 4>(r3, wl, 0, 0, L3.KB, L3.KB, PH2 + wave * CB3 * 512, CB3, lane, hacc);
            float y[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int col = nb * 16 + 4 * q + e;
                y[e] = hacc[0][0][e] + (col < No ? bl[L0.N + L1.N + L2.N + col] : 0.0f);
            }
            if (m < a.M && n.out) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (nb * 16 + 4 * q + e < No) n.out[(int64_t)m * n.ldo + nb * 16 + 4 * q + e] = y[e];
            }
            hook_head(wave, m, nb, y);
        }
    } else {
        hook_idle(extra);      // the wavefronts without a head block (NW - BM / 16 of them): free for the duration of the head
    }
    phase_stamp(a.dbg, 6);
}

template <int BM, int NW, int D, bool FIN = false>
__global__ __launch_bounds__(NW * 64) void mlp_fwd_kernel(const FwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (FIN && (int)blockIdx.y >= a.nets) {       // the extra grid row: the previous env step's finaliser, one workgroup
        if (blockIdx.x == 0) fin_block(a.fin, threadIdx.x, NW * 64);
        return;
    }
    const int which = a.net0 + blockIdx.y;
    const FusedNet& n = a.net[which];
    const int g1 = n.layer[0].NB / NW;     // first hidden width 256 / 512 / 768
    constexpr int U = 16 / NW;             // n-blocks per wave per 256 columns
    if (n.layer[3].NB > 1) {               // wide head: the auxiliary net (first hidden width 512 only)
        if (g1 == 2 * U) fwd_body<BM, NW, D, 2 * U, true>(a, n, false, smem);
        return;
    }
    if (g1 == 2 * U) fwd_body<BM, NW, D, 2 * U>(a, n, which == 0, smem);
    else if (g1 == 3 * U) fwd_body<BM, NW, D, 3 * U>(a, n, which == 0, smem);
    else if (g1 == U) fwd_body<BM, NW, D, U>(a, n, which == 0, smem);
}

// The forward with any resolved activation (GA): ONE net per launch (FwdArgs::net0, grid (tiles, 1)) and one kernel per first hidden
// width G1U * 256 / wide head, instead of mlp_fwd_kernel's dispatch over three or four tile bodies per kernel.  The GA epilogues are
// ~90 bytes of code per accumulator element against elu_bf's ~24, and a kernel that carries every body -- mlp_fwd_kernel is 72 .. 97 KB,
// mlp_fb_kernel 130 000 bytes -- would leave build.py's 128 KiB per kernel behind; these are 20 .. 45 KB each.  A postponed env-step
// finaliser is the caller's own launch here.
template <int BM, int NW, int D, int G1U, bool WIDE>
__global__ __launch_bounds__(NW * 64) void mlp_fwd_act_kernel(const FwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int U = 16 / NW;             // n-blocks per wave per 256 columns
    fwd_body<BM, NW, D, G1U * U, WIDE, false, false, true>(a, a.net[a.net0], !WIDE && a.net0 == 0, smem);
}

// ================================================================================================ backward (dX chain)
// dZ_out[m][k'] = (sum_n dZ_in[m][n] * W[n][k']) * elu'(H[m][k']): W^T fragments as the MFMA A operand.
// R: ring primed with this wave's first strip (bwd_prime); prime_next: called before the epilogue of the last strip.
template <int G, int D, int GR>
__device__ __forceinline__ void bwd_prime(WRing<GR, D>& R, const u32x4* __restrict__ WTf, int NBo, int NBBc, int wave, int lane) {
    const int nb0 = wave * G;
    if (nb0 < NBo) wring_prime<G, D>(R, WTf + (int64_t)nb0 * NBBc * 64 + lane, NBBc * 64, NBBc);
}

// HLDS / H_lds: the tile's y = elu(z) in LDS (block layout, NBo column blocks) instead of the global Hg -- the fused forward +
// backward kernel still has it there; out_lds may then be the SAME buffer (every lane reads a block entry and later writes that
// very entry).
// GA: f'(z) in Act's parametric form c0 + y (c1 - dq y) on the rounded y, exactly as act_bwd_tile takes it (no branch on the kind)
template <int G, int MB, int NW, int D, bool AHEAD, bool HLDS = false, bool GA = false, int GR, class Next>
__device__ __forceinline__ void bwd_step(WRing<GR, D>& R, const u32x4* __restrict__ WTf, int NBo, int NBBc, const char* in_lds, int CBin,
                                         char* out_lds, __bf16* __restrict__ dZg, const __bf16* __restrict__ Hg, int64_t mbg0, int wave,
                                         int lane, Next prime_next, const char* H_lds = nullptr, const Act* fn = nullptr) {
    const int r = lane & 15, q = lane >> 4;
    float d0p = 0.f, d1p = 0.f, d0n = 0.f, d1n = 0.f, ndq = 0.f;
    if constexpr (GA) { d0p = fn->d0p; d1p = fn->d1p; d0n = fn->d0n; d1n = fn->d1n; ndq = -fn->dq; }
    const int loff = r * 32 + q * 8;
    bool primed = false;
    for (int nb0 = wave * G; nb0 < NBo; nb0 += NW * G) {
        f32x4 acc[MB][G];
        zero_acc<G, MB>(acc);
        if (NBBc % D == 0) mma_stream<G, MB, D>(R, WTf + (int64_t)nb0 * NBBc * 64 + lane, NBBc * 64, NBBc, in_lds, CBin, lane, acc);
        else mma_ring<G, MB, D>(R, WTf + (int64_t)nb0 * NBBc * 64 + lane, NBBc * 64, 0, NBBc, NBBc, in_lds, CBin, lane, acc);
        const int nxt = nb0 + NW * G;
        if (nxt < NBo) wring_prime<G, D>(R, WTf + (int64_t)nxt * NBBc * 64 + lane, NBBc * 64, NBBc);
        else if (AHEAD) { prime_next(); primed = true; }
        u32x2 aux[MB][G];     // y = elu(z) of this tile (every load is issued before the first store below)
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (HLDS) aux[i][g] = *reinterpret_cast<const u32x2*>(H_lds + (i * NBo + nb0 + g) * 512 + loff);
                else aux[i][g] = ld_stream_u2<(kFusedNT & 4) != 0>(reinterpret_cast<const char*>(Hg) + ((mbg0 + i) * NBo + nb0 + g) * 512 + loff);
            }
        static_assert(MB % 2 == 0, "row blocks are stored in pairs");
#pragma unroll
        for (int i = 0; i < MB; i += 2)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                u32x2 pk[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const unsigned int w0 = aux[i + h][g][0], w1 = aux[i + h][g][1];
                    const float y[4] = {bf16_bits_to_f32(w0 & 0xffffu), bf16_bits_to_f32(w0 >> 16), bf16_bits_to_f32(w1 & 0xffffu),
                                        bf16_bits_to_f32(w1 >> 16)};
                    float d[4];
                    if constexpr (GA) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const bool p = y[e] > 0.0f;
                            d[e] = acc[i + h][g][e] * fmaf(y[e], fmaf(ndq, y[e], p ? d1p : d1n), p ? d0p : d0n);
                        }
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) d[e] = acc[i + h][g][e] * ((y[e] > 0.0f) ? 1.0f : (y[e] + 1.0f));   // elu'(z) from y = elu(z)
                    }
                    pk[h] = pack_bf16x4(d[0], d[1], d[2], d[3]);
                    if (out_lds) *reinterpret_cast<u32x2*>(out_lds + ((i + h) * NBo + nb0 + g) * 512 + loff) = pk[h];
                }
                char* pa = reinterpret_cast<char*>(dZg) + ((mbg0 + i) * NBo + nb0 + g) * 512 + loff;
                st_pair<(kFusedNT & 4) != 0, false>(pa, pa + (int64_t)NBo * 512, pk[0], pk[1], true, true, q);
            }
    }
    if (AHEAD && !primed) prime_next();
}

// ================================================================================================ forward + loss + dZ chain
// One kernel per minibatch instead of forward -> loss -> backward launches: a tile's
// forward leaves H1 and H2 in LDS (the two ping-pong buffers), the head wavefronts turn their outputs into the PPO loss gradient
// (the per-sample arithmetic of ppo_loss_kernel, one lane per (row, 4 actions)) -- dZ3 goes to LDS and to HBM -- and the dZ chain
// runs on the resident tile: through W3 against H2 (LDS, in place), through W2 against H1 (LDS, in place), through W1 against
// H0 (LDS: the forward is told to put H2 into a buffer of its own instead of over H0).
// HBM traffic per minibatch drops by the H re-reads and the loss kernel's own gathers; three launch boundaries go away.
// The loss partial row: what one loss workgroup (ppo_loss_kernel in hgym_loss.hpp, fb_body below) hands to ppo_scalars_block.
constexpr int LOSS_PARTIALS = 32;   // floats per loss workgroup: surrogate, value loss, entropy, kl, dstd[12], dbias_mu[12], dbias_v, aux, mirror, pad
enum { LP_SURROGATE = 0, LP_VALUE = 1, LP_ENTROPY = 2, LP_KL = 3, LP_DSTD = 4, LP_DBIAS_MU = 16, LP_DBIAS_V = 28, LP_AUX = 29, LP_MIRROR = 30 };
struct FbLoss {
    const float* actions;      // (T*N, A) storage columns, gathered through FwdArgs::idx
    const float* old_mu;
    const float* old_sigma;
    const float* values;       // (T*N,)
    const float* advantages;
    const float* returns;
    const float* logp;
    float clip, value_coef, entropy_coef;
    float* partials;           // [tiles][LOSS_PARTIALS] per-tile sums, the LP_* row: 0 surrogate, 1 value loss, 2 entropy, 3 kl,
                               // 4..15 d std, 16..27 sum d mu (head bias gradient), 28 sum d V, 29 the auxiliary head's squared error;
                               // the actor tile writes its entries, the critic tile its two, the auxiliary tile its one
    // auxiliary (denoising) head, a third grid row: MSE against columns [aux_off, aux_off + layer[3].N) of the gathered target rows
    const float* aux_target;
    int64_t aux_ldt;
    int aux_off;
    float aux_coef;
};

// The mirror loss (HgymPPOConfig.mirror_coef > 0): the argument of the FbMirror head's kernels only (hgym_update_mirror.hip,
// hgym_update_act_mirror.hip), so that FbLoss -- a kernel argument of every other update kernel -- keeps its layout.
struct FbMirror {
    const float* target;       // (M, A) fp32, row m of the MINIBATCH (contiguous, no gather): the raw mu of row m's partner (the pre-pass)
    const int32_t* act_src;    // (A,) M_a: t_j = act_sign[j] * target[m][act_src[j]]
    const float* act_sign;     // (A,)
    float g;                   // 2 * mirror_coef / (M * A): d L_m / d mu = g * (mu - t)
    int stage;                 // 1: the launch has FB_MIRROR_LDS more bytes of dynamic LDS behind fb_lds_bytes(net) and the tile's target rows
                               // and the table are staged there by the wavefronts idle in the third layer (with the other loss inputs)
};
constexpr int FB_MIRROR_LDS = 64 * 12 * 4 + 2 * 16 * 4;      // 64 rows x 12 floats, then act_src[16] (ints) and act_sign[16]

// The smoothness regulariser (hgym_ppo_grad_smooth): the argument of the FbSmooth head's kernels only (hgym_update_smooth.hip,
// hgym_update_act_smooth.hip), so that FbLoss and FbMirror keep their layouts.  Two detached targets and one weight per row of the MINIBATCH
// (contiguous, no gather): d mu += gT w (mu - tnext) + gS (mu - tnear).  A term whose g is 0 is off and its pointers are not read.
// An SM tile never carries the mirror loss, so the partial row's regression slot and the pad behind it are free for its two squared errors.
struct FbSmooth {
    const float* tnext;        // (M, A) fp32: mu of every row's successor (the temporal pre-pass)
    const float* tnear;        // (M, A) fp32: mu of every row's perturbed copy (the spatial pre-pass)
    const float* weight;       // (M,) 0 where the row has no successor, else 1
    float gT, gS;              // 2 * coef / (M * A)
    int stage;                 // 1: the launch has FB_SMOOTH_LDS more bytes of dynamic LDS behind fb_lds_bytes(net), and the tile's targets and
                               // weights are staged there by the wavefronts idle in the third layer
};
constexpr int LP_SMOOTH_T = LP_MIRROR, LP_SMOOTH_S = LP_MIRROR + 1;      // sum w |mu - tnext|^2, sum |mu - tnear|^2
static_assert(LP_SMOOTH_S < LOSS_PARTIALS, "the partial row has 32 floats");
constexpr int FB_SMOOTH_LDS = 2 * 64 * 12 * 4 + 64 * 4;      // tnext 64 x 12, tnear 64 x 12, weight 64

// Both at once (hgym_ppo_grad_smooth_mirror): the argument of the FbMirrorSmooth head's kernels only
// (hgym_update_mirror_smooth.hip, hgym_update_act_mirror_smooth.hip).  It holds the two heads' records as they are, so that every line of
// the tile that reads one of them is the line the single head runs: d mu = ((d mu_ppo + g (mu - M_a tm)) + gT w (mu - tT)) + gS (mu - tS).
// The partial row has two free slots for the actor and the combination has three sums: the mirror loss's squared error stays in LP_MIRROR
// (ppo_scalars_block turns it into HgymBatch.mirror_sums), the two smoothness errors of tile t go to head_partials[4 t], [4 t + 1].
struct FbMirrorSmooth {
    FbMirror m;                // (m.stage and s.stage repeat `stage`)
    FbSmooth s;
    float* head_partials;      // [tiles][4] fp32, caller-owned: sum w |mu - tnext|^2, sum |mu - tnear|^2, two floats never written
    int stage;                 // 1: the launch has FB_MIRROR_LDS + FB_SMOOTH_LDS more bytes of dynamic LDS behind fb_lds_bytes(net): the mirror
                               // head's block first, the smooth head's behind it
};
// where an MS tile's head waves leave the two smoothness sums in `red` for the cross-wave sum: slots of the row that an actor tile's waves
// never write (LP_AUX is the auxiliary tile's, the last float is pad); they leave LDS for head_partials, not for the partial row
constexpr int MS_RED_T = LP_AUX, MS_RED_S = LP_MIRROR + 1;

// Behaviour cloning (hgym_bc_grad): the argument of the FbBC head's kernels only (hgym_update_bc.hip, hgym_update_act_bc.hip).  The head
// regresses mu on target[row] -- a storage column gathered through FwdArgs::idx like every other loss input -- and nothing else: no
// surrogate, no entropy, no KL, no d std.  The tile's 64 target rows are staged in the actor's loss-input region of LDS (fb_lds_lin:
// 64 x FB_LIN_ACTOR floats, of which a row's first 12 are used), so a BC tile asks for exactly fb_lds_bytes(net).
struct FbBC {
    const float* target;       // (num_rows, A) fp32, 16-byte aligned rows when A == 12
    float inv;                 // 1 / (M * A)
    float delta;               // Huber's delta (> 0); unused by the MSE
    int huber;                 // 0: MSE, d mu = 2 e inv; 1: Huber, d mu = clamp(e, -delta, delta) inv
};

// Guidance by a frozen teacher (hgym_ppo_grad_guide): the argument of the FbGuide head's kernels only
// (hgym_update_guide.hip, hgym_update_act_guide.hip).  The PPO actor head plus c * inv2 * (mu - target[row]), the target a storage column
// gathered through FwdArgs::idx like every other loss input.  The coefficient c changes with every update of a captured graph, so it is
// read from the device -- one scalar load per tile -- and is no by-value argument.  A guided tile never carries the mirror loss: the squared
// error goes to the partial row's LP_MIRROR slot.
struct FbGuide {
    const float* target;       // (num_rows, A) fp32: the teacher's mean of every stored row; 16-byte aligned rows when A == 12
    const float* coef;         // one device float: this update's coefficient (hgym_guide_schedule)
    float inv2;                // 2 / (M * A): d L_g / d mu = coef * inv2 * (mu - t)
    int stage;                 // 1: the launch has FB_GUIDE_LDS more bytes of dynamic LDS behind fb_lds_bytes(net) and the tile's target rows are
                               // staged there by the wavefronts idle in the third layer (with the other loss inputs)
};
constexpr int FB_GUIDE_LDS = 64 * 12 * 4;      // 64 rows x 12 floats

// LDS of the fused kernel behind the forward's P / Q / bias regions: the dZ3 tile (64 rows x 32 * layer[3].NBB bf16 columns), the
// head waves' partial sums, and H2 (64 x layer[2].N bf16) -- the forward writes it there instead of over H0, so that all three
// activations are resident for the dZ chain
// ... and, behind H2, the storage row of each of the tile's 64 rows (256 B) and the loss inputs gathered through them: actor 64 x
// [actions 12 | old mu 12 | old sigma 12 | advantage | old log-prob | pad 2] floats, critic 64 x [return | old value]
constexpr int FB_LIN_ACTOR = 40;      // floats per row
HG_HD int fb_lds_lin(const FusedNet& n) { return n.layer[3].N == 1 ? 64 * 2 * 4 : (n.layer[3].N <= 12 ? 64 * FB_LIN_ACTOR * 4 : 0); }
HG_HD int fb_lds_extra(const FusedNet& n) { return 64 * 64 * n.layer[3].NBB + 4 * 32 * 4 + 64 * n.layer[2].N * 2 + 256 + fb_lds_lin(n); }

// Dynamic LDS the update's tiles of a net ask for, and the most a workgroup may have.  A net takes the fused path only if its
// mlp_fb_kernel tile fits (hgym_net.hip: fused_supported / fused_aux_supported, and the launch itself).  This also covers the forward:
// mlp_fwd_kernel's BM-row tile needs P + Q + bias (fwd_lds_bytes), which at 64 rows is a part of the same sum, and at 32 rows less.
constexpr size_t FB_LDS_LIMIT = 160 * 1024;
HG_HD int fwd_lds_bytes(const FusedNet& n, int BM) { return fused_lds_p(n, BM) + fused_lds_q(n, BM) + fused_lds_bias(n); }
HG_HD int fb_lds_bytes(const FusedNet& n) { return fwd_lds_bytes(n, 64) + fb_lds_extra(n); }
// the same from the net's widths (dims[0] = input .. dims[4] = head), before any workspace exists: the fields the sum reads,
// filled the way the workspace layout fills them (hgym_net.hip: ws_layout)
inline int fb_lds_bytes(const int32_t* dims) {
    FusedNet n{};
    for (int l = 0; l < 4; ++l) {
        n.layer[l].K = dims[l];
        n.layer[l].N = dims[l + 1];
        n.layer[l].NB = (dims[l + 1] + 15) / 16;
        n.layer[l].NBB = (dims[l + 1] + 31) / 32;
    }
    return fb_lds_bytes(n);
}

// The head of an update tile is a type.  FbPlain: the PPO head alone (actor: surrogate, entropy, KL; critic: value loss; AUX: the
// auxiliary head's MSE).  FbMirror / FbSmooth: the actor's PPO head with that term joined to d mu.  FbMirrorSmooth: with both.  FbBC: the
// actor's regression head.  FbGuide: the actor's PPO head with the teacher's term joined to d mu.
struct FbPlain {};
template <class T, class Head>      // H where the tile's head is a T (or, for FbMirrorSmooth, its record of that type), else null
__device__ __forceinline__ const T* head_as(const Head* H) {
    if constexpr (__is_same(T, Head)) return H;
    else if constexpr (__is_same(Head, FbMirrorSmooth) && __is_same(T, FbMirror)) return &H->m;
    else if constexpr (__is_same(Head, FbMirrorSmooth) && __is_same(T, FbSmooth)) return &H->s;
    else return nullptr;
}
// The slots of the partial row (LP_*) that a tile writes: each net's tiles their own, so that the launches of a minibatch do not meet.
template <class Head, bool AUX>
__device__ __forceinline__ constexpr bool fb_partial_mine(bool is_actor, int tid) {
    constexpr bool ML = __is_same(Head, FbMirror), BC = __is_same(Head, FbBC), SM = __is_same(Head, FbSmooth), MS = __is_same(Head, FbMirrorSmooth);
    constexpr bool GD = __is_same(Head, FbGuide);
    return BC    ? ((tid >= LP_DBIAS_MU && tid < LP_DBIAS_V) || tid == LP_MIRROR)      // d mu's sums and the regression slot
           : AUX ? tid == LP_AUX
                 : (is_actor ? ((tid != LP_VALUE && tid < LP_DBIAS_V) ||               // all of the PPO head's but the critic's two
                                ((ML || MS || GD) && tid == LP_MIRROR) ||
                                (SM && (tid == LP_SMOOTH_T || tid == LP_SMOOTH_S)))
                             : (tid == LP_VALUE || tid == LP_DBIAS_V));
}

// VU: the unclipped value loss (HgymPPOConfig.value_loss_unclipped); a template parameter, so that the clipped kernels stay as they were
// Head, *H: the tile's head and its arguments (null for FbPlain).  Every head-specific line stands under `if constexpr`, so each
// instantiation is what it would be without the others; the behaviour-cloning head has lambdas of its own (l2idle_bc, head_bc).
template <int G1, bool AUX = false, bool XB16 = false, bool VU = false, bool GA = false, class Head = FbPlain>
__device__ __forceinline__ void fb_body(const FwdArgs& a, const FbLoss& L, const FusedNet& n, bool is_actor, char* smem, const Head* H = nullptr) {
    constexpr bool ML = __is_same(Head, FbMirror), BC = __is_same(Head, FbBC), SM = __is_same(Head, FbSmooth);
    constexpr bool MS = __is_same(Head, FbMirrorSmooth);      // both heads: every ML line and every SM line, the SM block of LDS behind the ML one
    constexpr int SM_LDS0 = MS ? FB_MIRROR_LDS / 4 : 0;       // floats ahead of the smooth head's staged block
    constexpr bool GD = __is_same(Head, FbGuide);             // the teacher's term: gathered target rows, the coefficient from the device
    static_assert(__is_same(Head, FbPlain) || (!AUX && !VU), "a head other than the plain one is the actor's alone");
    const FbMirror* Mr = head_as<FbMirror>(H); const FbBC* Bc = head_as<FbBC>(H); const FbSmooth* Sm = head_as<FbSmooth>(H);
    const FbGuide* Gd = head_as<FbGuide>(H);
    constexpr int BM = 64, NW = 16, D = 2, MB = BM / 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int m0 = blockIdx.x * BM;
    const int64_t mbg0 = m0 >> 4;
    char* P = smem;
    char* Q = smem + fused_lds_p(n, BM);
    char* R0 = smem + fused_lds_p(n, BM) + fused_lds_q(n, BM) + fused_lds_bias(n);
    const int NBB3 = n.layer[3].NBB, CB3 = 2 * NBB3;      // the head gradient's column blocks of 16 (padded to the backward's k-steps of 32)
    float* red = reinterpret_cast<float*>(R0 + BM * 64 * NBB3);
    char* H2 = R0 + BM * 64 * NBB3 + 4 * 32 * 4;
    int* rowidx = reinterpret_cast<int*>(H2 + BM * n.layer[2].N * 2);
    float* lin = reinterpret_cast<float*>(rowidx + BM);
    const int A = a.A;
    // The loss inputs of the tile's rows (scattered 48-byte rows and scalars of the storage) are gathered into LDS by the eight
    // wavefronts that have no strip in the 128-wide third layer, while the other eight compute it: the head wavefronts used to
    // start with two dependent round trips (a.idx[m], then the rows) -- 5 of an actor tile's 47 us.
    const bool pre = !AUX && n.layer[2].NB <= 8 && (is_actor ? A == 12 : true);
    const float invB = 1.0f / (float)a.M;
    float aux_se = 0.0f;
    float guide_g = 0.0f;      // GD: coef * 2 / (M A), the coefficient read once per tile (a uniform address: one scalar load)
    if constexpr (GD) guide_g = Gd->coef[0] * Gd->inv2;
    // auxiliary head: lane (r, q) of head wave hw, row m, outputs nb * 16 + 4q .. + 3 (called once per column block).
    // loss = coef * mean_b sum_j (y - t)^2 / No, dL/dy = 2 coef (y - t) / (B No)    (aux_mse_kernel's arithmetic)
    auto head_aux = [&](int hw, int m, int nb, const float (&out)[4]) {
        const int No = n.layer[3].N;
        const bool valid = m < a.M;
        const int64_t row = rowidx[hw * 16 + r];
        const float* t = L.aux_target + row * L.aux_ldt + L.aux_off;
        const float gs = 2.0f * L.aux_coef / ((float)a.M * (float)No);
        float g[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = nb * 16 + 4 * q + e;
            float d = 0.0f;
            if (valid && j < No) {
                d = out[e] - t[j];
                aux_se += d * d;
            }
            g[e] = gs * d;
        }
        const u32x2 pk = pack_bf16x4(g[0], g[1], g[2], g[3]);
        const int off = (hw * CB3 + nb) * 512 + r * 32 + q * 8;
        char* gz = reinterpret_cast<char*>(n.dZ[3]) + mbg0 * CB3 * 512;
        *reinterpret_cast<u32x2*>(R0 + off) = pk;
        *reinterpret_cast<u32x2*>(gz + off) = pk;
        if (nb == 0) {      // the padding blocks behind the head's last one
            const u32x2 zero = {0u, 0u};
            for (int cb = n.layer[3].NB; cb < CB3; ++cb) {
                const int offz = (hw * CB3 + cb) * 512 + r * 32 + q * 8;
                *reinterpret_cast<u32x2*>(R0 + offz) = zero;
                *reinterpret_cast<u32x2*>(gz + offz) = zero;
            }
        }
    };
    auto l2idle = [&](int) {
        if (!pre) return;
        const int j = tid - 8 * 64;                 // 0 .. 511 (wavefronts 8 .. 15)
        if (j < 0) return;
        if constexpr (ML || MS) {
            // the tile's target rows (contiguous rows of the minibatch: no index to wait for) and M_a's table -> LDS, beside the other
            // loss inputs: the head reads them there, one LDS access behind another instead of two dependent trips to memory
            if (Mr->stage) {
                float* mt = lin + FB_LIN_ACTOR * 64;
                const int rw = j / 3 < 63 ? j / 3 : 63, k = j % 3;
                int mrow = m0 + rw;
                mrow = mrow < a.M ? mrow : a.M - 1;
                const F4 vt = *reinterpret_cast<const F4*>(Mr->target + (int64_t)mrow * 12 + 4 * k);
                const int tj = j & 15;
                const int sv = Mr->act_src[tj < 12 ? tj : 0];
                const float gv = Mr->act_sign[tj < 12 ? tj : 0];
                if (j < 192) *reinterpret_cast<F4*>(mt + rw * 12 + 4 * k) = vt;
                if (j >= 192 && j < 208) reinterpret_cast<int*>(mt + 64 * 12)[tj] = sv < 0 ? 0 : (sv > 11 ? 11 : sv);
                if (j >= 208 && j < 224) mt[64 * 12 + 16 + tj] = gv;
            }
        }
        if constexpr (SM || MS) {
            // the tile's two target blocks and its weights (contiguous rows of the minibatch) -> LDS behind the other loss inputs: lanes
            // 0 .. 191 the temporal targets, 192 .. 383 the spatial ones, 384 .. 447 the weights.  A term that is off is neither read nor
            // staged (its pointers may be null): the load goes to the other term's block instead, the store is skipped.  Invariant: at
            // least one term is on -- with both off the host launches the plain tile, never this kernel -- so `src` below is never null.
            // Rows of 12 floats: l2idle runs under `pre` only, which for the actor means A == 12 (FB_SMOOTH_LDS is sized for that).
            // (Lanes 384 .. 511 also issue the 16-byte load, of row 63, and drop it: unconditional loads, conditional stores, as above.)
            if (Sm->stage) {
                float* st = lin + FB_LIN_ACTOR * 64 + SM_LDS0;
                const bool onT = Sm->gT > 0.0f, onS = Sm->gS > 0.0f;
                const bool second = j >= 192;
                const int jj = second ? j - 192 : j;
                const int rw = jj / 3 < 63 ? jj / 3 : 63, k = jj % 3;
                int mrow = m0 + rw;
                mrow = mrow < a.M ? mrow : a.M - 1;
                const float* src = (second ? onS : !onT) ? Sm->tnear : Sm->tnext;
                const F4 vt = *reinterpret_cast<const F4*>(src + (int64_t)mrow * 12 + 4 * k);
                int wrow = m0 + (j & 63);
                wrow = wrow < a.M ? wrow : a.M - 1;
                const float wv = onT ? Sm->weight[wrow] : 0.0f;
                if (j < 384 && (second ? onS : onT)) *reinterpret_cast<F4*>(st + (second ? 64 * 12 : 0) + rw * 12 + 4 * k) = vt;
                if (j >= 384 && j < 448) st[2 * 64 * 12 + (j & 63)] = wv;
            }
        }
        if constexpr (GD) {
            // the tile's 64 target rows, gathered through rowidx like the actions (three 16-byte loads per row), -> LDS behind the other
            // loss inputs.  Rows of 12 floats: l2idle runs under `pre` only, which for the actor means A == 12.
            if (Gd->stage) {
                float* gt = lin + FB_LIN_ACTOR * 64;
                const int rw = j / 3 < 63 ? j / 3 : 63, k = j % 3;
                const int64_t ri = rowidx[rw];
                const F4 vt = *reinterpret_cast<const F4*>(Gd->target + ri * 12 + 4 * k);
                if (j < 192) *reinterpret_cast<F4*>(gt + rw * 12 + 4 * k) = vt;
            }
        }
        if (is_actor) {
            // round 1: (row, quad k): actions 0..2, old mu 3..5, old sigma 6..7; round 2: old sigma quad 2, advantage, old log-prob.
            // Every load is issued before the first LDS write.
            const int rw = j >> 3, k = j & 7;
            const int64_t ri = rowidx[rw];
            const float* base = k < 3 ? L.actions : (k < 6 ? L.old_mu : L.old_sigma);
            const F4 v1 = *reinterpret_cast<const F4*>(base + ri * 12 + 4 * (k < 3 ? k : (k < 6 ? k - 3 : k - 6)));
            // (unconditional loads, conditional stores: a conditionally initialised vector ends up in private memory)
            const int rw2 = j & 63;
            const int64_t ri2 = rowidx[rw2];
            const F4 v2 = *reinterpret_cast<const F4*>(L.old_sigma + ri2 * 12 + 8);
            const float s2 = (j < 128 ? L.advantages : L.logp)[ri2];
            *reinterpret_cast<F4*>(lin + rw * FB_LIN_ACTOR + 4 * k) = v1;
            if (j < 64) *reinterpret_cast<F4*>(lin + rw2 * FB_LIN_ACTOR + 32) = v2;
            else if (j < 192) lin[rw2 * FB_LIN_ACTOR + (j < 128 ? 36 : 37)] = s2;
        } else if (j < 128) {
            const int rw = j & 63;
            const int64_t ri = rowidx[rw];
            lin[rw * 2 + (j >> 6)] = j < 64 ? L.returns[ri] : L.values[ri];
        }
    };
    auto head = [&](int hw, int m, int, const float (&out)[4]) {
        // lane (r, q) of head wave hw: row m, head outputs 4q .. 4q + 3.  ppo.py:128-168 forward scalars + the hand-written
        // backward of the loss w.r.t. mu, std and V (oracle/ppo_oracle.py: ppo_loss_and_grads), as in ppo_loss_kernel
        const bool valid = m < a.M;
        const int rl = hw * 16 + r;                 // row of the tile
        const int64_t row = rowidx[rl];
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        constexpr int NPART = MS ? 14 : ((ML || GD) ? 12 : (SM ? 13 : 11));      // ML: [11] the mirror loss's squared error; SM: [11], [12] the two terms'; MS: [11], then [12], [13]; GD: [11] the teacher's
        constexpr int PT = MS ? 12 : 11;                        // the temporal term's sum, the spatial term's behind it
        float part[NPART];
#pragma unroll
        for (int k = 0; k < NPART; ++k) part[k] = 0.0f;
        if (is_actor) {
            float act[4] = {0.f, 0.f, 0.f, 0.f}, mo[4] = {0.f, 0.f, 0.f, 0.f}, so[4] = {1.f, 1.f, 1.f, 1.f}, sg[4] = {1.f, 1.f, 1.f, 1.f};
            if (pre) {
                if (q < 3) {
                    const F4 qa = *reinterpret_cast<const F4*>(lin + rl * FB_LIN_ACTOR + 4 * q);
                    const F4 qo = *reinterpret_cast<const F4*>(lin + rl * FB_LIN_ACTOR + 12 + 4 * q);
                    const F4 qs = *reinterpret_cast<const F4*>(lin + rl * FB_LIN_ACTOR + 24 + 4 * q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { act[e] = qa.v[e]; mo[e] = qo.v[e]; so[e] = qs.v[e]; }
                }
            } else if (4 * q + 3 < A) {
                const F4 qa = *reinterpret_cast<const F4*>(L.actions + row * A + 4 * q);
                const F4 qo = *reinterpret_cast<const F4*>(L.old_mu + row * A + 4 * q);
                const F4 qs = *reinterpret_cast<const F4*>(L.old_sigma + row * A + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) { act[e] = qa.v[e]; mo[e] = qo.v[e]; so[e] = qs.v[e]; }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * q + e < A) { act[e] = L.actions[row * A + 4 * q + e]; mo[e] = L.old_mu[row * A + 4 * q + e]; so[e] = L.old_sigma[row * A + 4 * q + e]; }
            }
            const float adv = pre ? lin[rl * FB_LIN_ACTOR + 36] : L.advantages[row], lpold = pre ? lin[rl * FB_LIN_ACTOR + 37] : L.logp[row];
            float lp = 0.0f, ent = 0.0f, kl = 0.0f, diff[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                diff[e] = 0.0f;
                if (4 * q + e < A) {
                    const float mm = out[e];
                    const float s = mm * 0.0f + a.std_[4 * q + e];
                    const float d = act[e] - mm;
                    diff[e] = d;
                    sg[e] = s;
                    lp += -(d * d) / (2.0f * s * s) - logf(s) - 0.9189385332046727f;
                    ent += 0.5f + 0.9189385332046727f + logf(s);
                    if constexpr (MS) {
                        // The one sum of two products in the head: which of them the compiler fuses into the add is its choice per
                        // instantiation.  Every other tile forms fma(so, so, (mo - mm)^2); left to itself this one fuses the other
                        // product, and the KL partial -- which must keep hgym_ppo_grad's bits -- moves in its last place.  So it is spelt out.
                        kl += logf(s / so[e] + 1.e-5f) + __builtin_fmaf(so[e], so[e], (mo[e] - mm) * (mo[e] - mm)) / (2.0f * (s * s)) - 0.5f;
                    } else {
                        kl += logf(s / so[e] + 1.e-5f) + (so[e] * so[e] + (mo[e] - mm) * (mo[e] - mm)) / (2.0f * (s * s)) - 0.5f;
                    }
                }
            }
            lp += __shfl_xor(lp, 16, 64);  lp += __shfl_xor(lp, 32, 64);
            ent += __shfl_xor(ent, 16, 64); ent += __shfl_xor(ent, 32, 64);
            kl += __shfl_xor(kl, 16, 64);  kl += __shfl_xor(kl, 32, 64);
            const float ratio = expf(lp - lpold);
            const float s1 = -adv * ratio;
            const float s2 = -adv * clampf(ratio, 1.0f - L.clip, 1.0f + L.clip);
            const float in_range = (ratio >= 1.0f - L.clip && ratio <= 1.0f + L.clip) ? 1.0f : 0.0f;
            const float w1 = s1 > s2 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f);
            const float d_lp = (-adv) * (w1 + (1.0f - w1) * in_range) * invB * ratio;
            if (valid) {
                if (q == 0) { part[0] = fmaxf(s1, s2); part[1] = ent; part[2] = kl; }
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * q + e < A) {
                        const float s = sg[e], d = diff[e];
                        g[e] = d_lp * d / (s * s);
                        part[3 + e] = d_lp * (d * d / (s * s * s) - 1.0f / s) - (L.entropy_coef * invB) / s;
                        part[7 + e] = g[e];
                    }
            }
            if constexpr (ML || MS) {
                // the mirror loss: g (mu - t) joins d mu (and the head-bias sum), (mu - t)^2 the tile's partial sum; nothing else moves
                const bool staged = pre && Mr->stage;
                const float* mt = lin + FB_LIN_ACTOR * 64;
                const int mrow = valid ? m : a.M - 1;
                float se = 0.0f;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * q + e < A) {
                        float t;
                        if (staged) {
                            t = mt[64 * 12 + 16 + 4 * q + e] * mt[rl * 12 + reinterpret_cast<const int*>(mt + 64 * 12)[4 * q + e]];
                        } else {
                            int sj = Mr->act_src[4 * q + e];
                            sj = sj < 0 ? 0 : (sj >= A ? A - 1 : sj);
                            t = Mr->act_sign[4 * q + e] * Mr->target[(int64_t)mrow * A + sj];
                        }
                        const float dm = out[e] - t;
                        if (valid) {
                            g[e] += Mr->g * dm;
                            part[7 + e] = g[e];
                            se += dm * dm;
                        }
                    }
                se += __shfl_xor(se, 16, 64); se += __shfl_xor(se, 32, 64);
                if (q == 0) part[11] = se;
            }
            if constexpr (SM || MS) {
                // the smoothness terms: gT w (mu - tnext) + gS (mu - tnear) joins d mu (and the head-bias sum), the two squared errors the
                // tile's partial sums; nothing else moves.  A term that is off reads nothing.
                const bool staged = pre && Sm->stage;
                const float* st = lin + FB_LIN_ACTOR * 64 + SM_LDS0;
                const int mrow = valid ? m : a.M - 1;
                const bool onT = Sm->gT > 0.0f, onS = Sm->gS > 0.0f;
                const float wgt = onT ? (staged ? st[2 * 64 * 12 + rl] : Sm->weight[mrow]) : 0.0f;
                float seT = 0.0f, seS = 0.0f;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * q + e < A) {
                        if (onT) {
                            const float t = staged ? st[rl * 12 + 4 * q + e] : Sm->tnext[(int64_t)mrow * A + 4 * q + e];
                            const float dm = out[e] - t;
                            if (valid) {
                                g[e] += Sm->gT * wgt * dm;
                                seT += wgt * dm * dm;
                            }
                        }
                        if (onS) {
                            const float t = staged ? st[64 * 12 + rl * 12 + 4 * q + e] : Sm->tnear[(int64_t)mrow * A + 4 * q + e];
                            const float dm = out[e] - t;
                            if (valid) {
                                g[e] += Sm->gS * dm;
                                seS += dm * dm;
                            }
                        }
                        if (valid) part[7 + e] = g[e];
                    }
                seT += __shfl_xor(seT, 16, 64); seT += __shfl_xor(seT, 32, 64);
                seS += __shfl_xor(seS, 16, 64); seS += __shfl_xor(seS, 32, 64);
                if (q == 0) { part[PT] = seT; part[PT + 1] = seS; }
            }
            if constexpr (GD) {
                // the teacher's term: c inv2 (mu - t) joins d mu (and the head-bias sum), (mu - t)^2 the tile's partial sum; nothing else moves
                const bool staged = pre && Gd->stage;
                const float* gt = lin + FB_LIN_ACTOR * 64;
                float se = 0.0f;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * q + e < A) {
                        const float t = staged ? gt[rl * 12 + 4 * q + e] : Gd->target[row * A + 4 * q + e];
                        const float dm = out[e] - t;
                        if (valid) {
                            g[e] += guide_g * dm;
                            part[7 + e] = g[e];
                            se += dm * dm;
                        }
                    }
                se += __shfl_xor(se, 16, 64); se += __shfl_xor(se, 32, 64);
                if (q == 0) part[11] = se;
            }
        } else {
            const float ret = pre ? lin[rl * 2] : L.returns[row], vold = pre ? lin[rl * 2 + 1] : L.values[row];
            const float v = out[0];
            if constexpr (VU) {         // (R - V)^2: the stored old value plays no part
                (void)vold;
                if (valid && q == 0) {
                    g[0] = L.value_coef * invB * (2.0f * (v - ret));
                    part[0] = (v - ret) * (v - ret);
                    part[1] = g[0];
                }
            } else {
                const float vc = vold + clampf(v - vold, -L.clip, L.clip);
                const float l1 = (v - ret) * (v - ret), l2 = (vc - ret) * (vc - ret);
                const float v_in = ((v - vold) >= -L.clip && (v - vold) <= L.clip) ? 1.0f : 0.0f;
                const float u1 = l1 > l2 ? 1.0f : (l1 == l2 ? 0.5f : 0.0f);
                if (valid && q == 0) {
                    g[0] = L.value_coef * invB * (u1 * 2.0f * (v - ret) + (1.0f - u1) * 2.0f * (vc - ret) * v_in);
                    part[0] = fmaxf(l1, l2);
                    part[1] = g[0];
                }
            }
        }
        // dZ3 tile, block layout: row block hw, column block 0 holds this lane's 4 columns (block 1 is zero padding)
        const u32x2 pk = pack_bf16x4(g[0], g[1], g[2], g[3]);
        const u32x2 zero = {0u, 0u};
        const int off0 = (hw * 2 + 0) * 512 + r * 32 + q * 8, off1 = (hw * 2 + 1) * 512 + r * 32 + q * 8;
        *reinterpret_cast<u32x2*>(R0 + off0) = pk;
        *reinterpret_cast<u32x2*>(R0 + off1) = zero;
        char* gz = reinterpret_cast<char*>(n.dZ[3]) + mbg0 * 2 * 512;
        *reinterpret_cast<u32x2*>(gz + off0) = pk;
        *reinterpret_cast<u32x2*>(gz + off1) = zero;
        // sums over the 16 rows of this wave (lanes sharing q), then across the head waves through `red`
#pragma unroll
        for (int k = 0; k < NPART; ++k) {
            float v = part[k];
            v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
            part[k] = v;
        }
        if (r == 0) {
            float* w = red + hw * LOSS_PARTIALS;
            if (is_actor) {
                if (q == 0) { w[LP_SURROGATE] = part[0]; w[LP_ENTROPY] = part[1]; w[LP_KL] = part[2]; }
                if constexpr (ML || MS || GD) { if (q == 0) w[LP_MIRROR] = part[11]; }
                if constexpr (SM) { if (q == 0) { w[LP_SMOOTH_T] = part[11]; w[LP_SMOOTH_S] = part[12]; } }
                if constexpr (MS) { if (q == 0) { w[MS_RED_T] = part[PT]; w[MS_RED_S] = part[PT + 1]; } }
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * q + e < 12) { w[LP_DSTD + 4 * q + e] = part[3 + e]; w[LP_DBIAS_MU + 4 * q + e] = part[7 + e]; }
            } else if (q == 0) {
                w[LP_VALUE] = part[0];
                w[LP_DBIAS_V] = part[1];
            }
        }
    };
    // Behaviour cloning.  l2idle_bc: wavefronts 8 .. 15 bring the tile's 64 target rows (three 16-byte loads per row, gathered through
    // rowidx) into lin[row * 12 ..] while the other eight compute the third layer.  head_bc: lane (r, q) of head wave hw holds outputs
    // 4q .. 4q + 3 of row m: e = mu - t, d mu and the row's loss terms; dZ3 and the partial row leave as in `head`.
    auto l2idle_bc = [&](int) {
        if (!pre) return;
        const int j = tid - 8 * 64;
        if (j < 0 || j >= 192) return;
        const int rw = j / 3, k = j - 3 * rw;
        const int64_t ri = rowidx[rw];
        const F4 vt = *reinterpret_cast<const F4*>(Bc->target + ri * 12 + 4 * k);
        *reinterpret_cast<F4*>(lin + rw * 12 + 4 * k) = vt;
    };
    auto head_bc = [&](int hw, int m, int, const float (&out)[4]) {
        const bool valid = m < a.M;
        const int rl = hw * 16 + r;
        const int64_t row = rowidx[rl];
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        float part[5] = {0.f, 0.f, 0.f, 0.f, 0.f};      // [0] the loss terms, [1 + e] d mu of output 4q + e
        float ls = 0.0f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = 4 * q + e;
            if (j < A) {
                const float t = pre ? lin[rl * 12 + j] : Bc->target[row * A + j];
                const float d = out[e] - t;
                float gd, le;
                if (Bc->huber) {
                    const float ad = fabsf(d);
                    gd = clampf(d, -Bc->delta, Bc->delta);
                    le = ad <= Bc->delta ? 0.5f * d * d : Bc->delta * (ad - 0.5f * Bc->delta);
                } else {
                    gd = 2.0f * d;
                    le = d * d;
                }
                if (valid) {
                    g[e] = gd * Bc->inv;
                    part[1 + e] = g[e];
                    ls += le;
                }
            }
        }
        ls += __shfl_xor(ls, 16, 64); ls += __shfl_xor(ls, 32, 64);
        if (q == 0) part[0] = ls;
        const u32x2 pk = pack_bf16x4(g[0], g[1], g[2], g[3]);
        const u32x2 zero = {0u, 0u};
        const int off0 = (hw * 2 + 0) * 512 + r * 32 + q * 8, off1 = (hw * 2 + 1) * 512 + r * 32 + q * 8;
        *reinterpret_cast<u32x2*>(R0 + off0) = pk;
        *reinterpret_cast<u32x2*>(R0 + off1) = zero;
        char* gz = reinterpret_cast<char*>(n.dZ[3]) + mbg0 * 2 * 512;
        *reinterpret_cast<u32x2*>(gz + off0) = pk;
        *reinterpret_cast<u32x2*>(gz + off1) = zero;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            float v = part[k];
            v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
            part[k] = v;
        }
        if (r == 0) {
            float* w = red + hw * LOSS_PARTIALS;
            if (q == 0) w[LP_MIRROR] = part[0];      // the partial row's regression slot: the behaviour loss here, the mirror loss in an ML tile
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * q + e < 12) w[LP_DBIAS_MU + 4 * q + e] = part[1 + e];
        }
    };
    if constexpr (BC) {
        fwd_body<BM, NW, D, G1, false, XB16, false, GA>(a, n, true, smem, FwdNoop(), FwdNoop(), FwdNoop(), 0, FwdNoop(), head_bc, H2, rowidx, l2idle_bc);
    } else if constexpr (AUX) {
        fwd_body<BM, NW, D, G1, true, XB16, false, GA>(a, n, false, smem, FwdNoop(), FwdNoop(), FwdNoop(), 0, FwdNoop(), head_aux, H2, rowidx);
        if (wave < MB) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) aux_se += __shfl_xor(aux_se, o, 64);
            if (lane == 0) red[wave * LOSS_PARTIALS + LP_AUX] = aux_se;
        }
    } else {
        fwd_body<BM, NW, D, G1, false, XB16, false, GA>(a, n, is_actor, smem, FwdNoop(), FwdNoop(), FwdNoop(), 0, FwdNoop(), head, H2, rowidx, l2idle);
    }
    __syncthreads();          // dZ3 tile and the per-wave sums are in LDS; H0 sits in P, H1 in Q, H2 in its own buffer
    if (tid < LOSS_PARTIALS) {
        const bool mine = fb_partial_mine<Head, AUX>(is_actor, tid);
        if (mine) L.partials[(int64_t)blockIdx.x * LOSS_PARTIALS + tid] = red[tid] + red[LOSS_PARTIALS + tid] + red[2 * LOSS_PARTIALS + tid] + red[3 * LOSS_PARTIALS + tid];
        if constexpr (MS) {      // the tile's two smoothness sums, added across the head waves as the partial row's slots are
            if (tid == MS_RED_T || tid == MS_RED_S)
                H->head_partials[(int64_t)blockIdx.x * 4 + (tid == MS_RED_S ? 1 : 0)] = red[tid] + red[LOSS_PARTIALS + tid] + red[2 * LOSS_PARTIALS + tid] + red[3 * LOSS_PARTIALS + tid];
        }
    }
    // ---- dZ chain on the resident tile
    const int N0 = n.layer[0].N, N1 = n.layer[1].N, N2 = n.layer[2].N;
    WRing<1, D> ra;
    WRing<1, D> rb;
    WRing<G1, D> rc;
    auto none = [&]() {};
    bwd_prime<1, D>(ra, n.layer[3].WTf, N2 / 16, NBB3, wave, lane);
    bwd_step<1, MB, NW, D, false, true, GA>(ra, n.layer[3].WTf, N2 / 16, NBB3, R0, 2 * NBB3, H2, n.dZ[2], nullptr, mbg0, wave, lane, none, H2, &a.act);
    __syncthreads();
    bwd_prime<1, D>(rb, n.layer[2].WTf, N1 / 16, n.layer[2].NBB, wave, lane);
    bwd_step<1, MB, NW, D, false, true, GA>(rb, n.layer[2].WTf, N1 / 16, n.layer[2].NBB, H2, N2 / 16, Q, n.dZ[1], nullptr, mbg0, wave, lane, none, Q, &a.act);
    __syncthreads();
    bwd_prime<G1, D>(rc, n.layer[1].WTf, N0 / 16, n.layer[1].NBB, wave, lane);
    bwd_step<G1, MB, NW, D, false, true, GA>(rc, n.layer[1].WTf, N0 / 16, n.layer[1].NBB, Q, N1 / 16, nullptr, n.dZ[0], nullptr, mbg0, wave, lane, none, P, &a.act);
    phase_stamp(a.dbg, 7);
}

// XB16: every net of the launch gathers its input rows from the bf16 shadow (FusedNet::xb) instead of the fp32 storage rows
// VU: the critic tile forms the unclipped value loss (R - V)^2 (HgymPPOConfig.value_loss_unclipped)
template <bool XB16 = false, bool VU = false>
__global__ __launch_bounds__(1024) void mlp_fb_kernel(const FwdArgs a, const FbLoss L) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int which = a.net0 + blockIdx.y;
    const FusedNet& n = a.net[which];
    const int g1 = n.layer[0].NB / 16;     // first hidden width 256 / 512 / 768
    if (which == 2) {                      // the auxiliary head (wide head, first hidden width 512 only): MSE instead of the PPO loss
        if (g1 == 2) fb_body<2, true, XB16, VU>(a, L, n, false, smem);
        return;
    }
    if (g1 == 2) fb_body<2, false, XB16, VU>(a, L, n, which == 0, smem);
    else if (g1 == 3) fb_body<3, false, XB16, VU>(a, L, n, which == 0, smem);
    else if (g1 == 1) fb_body<1, false, XB16, VU>(a, L, n, which == 0, smem);
}

// One launch of mlp_fb_kernel<shadow, VU>.  Each value-loss form lives in a translation unit of its own (hgym_update.hip: clipped,
// hgym_update_vu.hip: unclipped), so that neither device code object grows by the other's two 125 KB kernels.
template <bool VU>
int32_t launch_mlp_fb_form(const FwdArgs& fb, const FbLoss& fl, bool shadow, int tiles, int nets, size_t lds, hipStream_t s) {
    const int32_t rc = shadow ? ensure_dynamic_lds(reinterpret_cast<const void*>(&mlp_fb_kernel<true, VU>), lds, "mlp_fb_kernel<shadow>")
                              : ensure_dynamic_lds(reinterpret_cast<const void*>(&mlp_fb_kernel<false, VU>), lds, "mlp_fb_kernel");
    if (rc) return rc;
    if (shadow) hipLaunchKernelGGL((mlp_fb_kernel<true, VU>), dim3(tiles, nets), dim3(1024), lds, s, fb, fl);
    else hipLaunchKernelGGL((mlp_fb_kernel<false, VU>), dim3(tiles, nets), dim3(1024), lds, s, fb, fl);
    return HGYM_OK;
}

// The update tile with any resolved activation (GA): one net per launch and one kernel per tile body, for the reason given at
// mlp_fwd_act_kernel (mlp_fb_kernel<false, false> is 130 000 bytes of the 131 072 a kernel may have).  Every net's tiles write their own
// entries of the per-tile partial sums, so the launches of a minibatch are independent of each other.
template <int G1, bool AUX, bool XB16, bool VU>
__global__ __launch_bounds__(1024) void mlp_fb_act_kernel(const FwdArgs a, const FbLoss L) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fb_body<G1, AUX, XB16, VU, true>(a, L, a.net[a.net0], !AUX && a.net0 == 0, smem);
}

template <int G1, bool AUX, bool VU>
int32_t launch_mlp_fb_act_one(const FwdArgs& fb, const FbLoss& fl, bool shadow, int tiles, size_t lds, hipStream_t s) {
    const int32_t rc = shadow ? ensure_dynamic_lds(reinterpret_cast<const void*>(&mlp_fb_act_kernel<G1, AUX, true, VU>), lds, "mlp_fb_act_kernel<shadow>")
                              : ensure_dynamic_lds(reinterpret_cast<const void*>(&mlp_fb_act_kernel<G1, AUX, false, VU>), lds, "mlp_fb_act_kernel");
    if (rc) return rc;
    if (shadow) hipLaunchKernelGGL((mlp_fb_act_kernel<G1, AUX, true, VU>), dim3(tiles), dim3(1024), lds, s, fb, fl);
    else hipLaunchKernelGGL((mlp_fb_act_kernel<G1, AUX, false, VU>), dim3(tiles), dim3(1024), lds, s, fb, fl);
    return HGYM_OK;
}
// the launches of mlp_fb_act_kernel for nets [0, nets) of fb0 (hgym_update_act.hip: clipped value loss, hgym_update_act_vu.hip: unclipped)
// first: the first net launched (1: the actor's tiles have their own launch, launch_mlp_fb_head)
template <bool VU>
int32_t launch_mlp_fb_act_form(const FwdArgs& fb0, const FbLoss& fl, bool shadow, int tiles, int nets, hipStream_t s, int first = 0) {
    for (int i = first; i < nets; ++i) {
        FwdArgs fb = fb0;
        fb.net0 = i;
        fb.nets = 1;
        if (fb.dbg) fb.dbg += (int64_t)i * tiles * 8;      // phase stamps: this net's slots
        const size_t lds = (size_t)fb_lds_bytes(fb.net[i]);
        const int g1 = fb.net[i].layer[0].NB / 16;         // first hidden width 256 / 512 / 768
        int32_t rc = HGYM_E_UNSUPPORTED;
        if (i == 2) rc = launch_mlp_fb_act_one<2, true, VU>(fb, fl, shadow, tiles, lds, s);      // the auxiliary head: first width 512
        else if (g1 == 1) rc = launch_mlp_fb_act_one<1, false, VU>(fb, fl, shadow, tiles, lds, s);
        else if (g1 == 2) rc = launch_mlp_fb_act_one<2, false, VU>(fb, fl, shadow, tiles, lds, s);
        else if (g1 == 3) rc = launch_mlp_fb_act_one<3, false, VU>(fb, fl, shadow, tiles, lds, s);
        if (rc) return rc;
    }
    return HGYM_OK;
}

// The ACTOR's update tile with a head of its own (FbMirror: HgymPPOConfig.mirror_coef > 0, FbSmooth: hgym_ppo_grad_smooth, FbMirrorSmooth:
// hgym_ppo_grad_smooth_mirror, FbBC: hgym_bc_grad): one kernel per head, first hidden width, input form and activation form (GA), the actor alone.  Beside the mirror and
// the smooth tiles the critic's and the auxiliary head's tiles run through the kernels they always had (mlp_fb_kernel from net 1 on,
// launch_mlp_fb_act_form with first = 1), so those nets' bits cannot move; a cloning step has no other net.  The head is THIS kernel's
// third argument, so that FbLoss -- an argument of every other update kernel -- keeps its layout.
template <class Head, int G1, bool XB16, bool GA>
__global__ __launch_bounds__(1024) void mlp_fb_head_kernel(const FwdArgs a, const FbLoss L, const Head head) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fb_body<G1, false, XB16, false, GA, Head>(a, L, a.net[0], true, smem, &head);
}
// The cloning head's kernel is mlp_fb_head_kernel<FbBC, ..> under the name it came with.  A kernel's name is part of its code object:
// its length decides where the kernel descriptors come to lie, and the change that gave the heads one template moved no byte of any
// code object's .text or .rodata (tools/code_identity.py).  Whatever next moves this code anyway can drop this template.
template <int G1, bool XB16, bool GA>
__global__ __launch_bounds__(1024) void mlp_fb_bc_kernel(const FwdArgs a, const FbLoss L, const FbBC bc) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fb_body<G1, false, XB16, false, GA, FbBC>(a, L, a.net[0], true, smem, &bc);
}
template <class Head, int G1, bool XB16, bool GA>
auto fb_head_kernel() {
    if constexpr (__is_same(Head, FbBC)) return &mlp_fb_bc_kernel<G1, XB16, GA>;
    else return &mlp_fb_head_kernel<Head, G1, XB16, GA>;
}

// What the launch knows about a head: the dynamic LDS it stages its targets in behind fb_lds_bytes(net), the field that says so
// (`stage`), and its name in an error message.
inline int fb_head_lds(const FbMirror&) { return FB_MIRROR_LDS; }
inline int fb_head_lds(const FbSmooth&) { return FB_SMOOTH_LDS; }
inline int fb_head_lds(const FbMirrorSmooth&) { return FB_MIRROR_LDS + FB_SMOOTH_LDS; }
inline int fb_head_lds(const FbGuide&) { return FB_GUIDE_LDS; }
inline int fb_head_lds(const FbBC&) { return 0; }      // its targets lie in the loss-input region the sum already holds
inline void fb_head_stage(FbMirror& h, int on) { h.stage = on; }
inline void fb_head_stage(FbSmooth& h, int on) { h.stage = on; }
inline void fb_head_stage(FbMirrorSmooth& h, int on) { h.stage = h.m.stage = h.s.stage = on; }
inline void fb_head_stage(FbGuide& h, int on) { h.stage = on; }
inline void fb_head_stage(FbBC&, int) {}
inline const char* fb_head_name(const FbMirror&) { return "mlp_fb_head_kernel<mirror>"; }
inline const char* fb_head_name(const FbSmooth&) { return "mlp_fb_head_kernel<smooth>"; }
inline const char* fb_head_name(const FbMirrorSmooth&) { return "mlp_fb_head_kernel<mirror_smooth>"; }
inline const char* fb_head_name(const FbGuide&) { return "mlp_fb_head_kernel<guide>"; }
inline const char* fb_head_name(const FbBC&) { return "mlp_fb_bc_kernel"; }

// One launch of the actor's tiles with `head0`.  Each (GA, Head) is explicitly instantiated in a translation unit, i.e. a device code
// object, of its own (hgym_update_{mirror,smooth,mirror_smooth,guide,bc}.hip: ELU(1), hgym_update_act_{..}.hip: any resolved activation) and
// declared `extern` below: no other translation unit carries these kernels.
template <bool GA, class Head>
int32_t launch_mlp_fb_head(const FwdArgs& fb0, const FbLoss& fl, const Head& head0, bool shadow, int tiles, hipStream_t s) {
    FwdArgs fb = fb0;
    fb.net0 = 0;
    fb.nets = 1;
    Head head = head0;
    size_t lds = (size_t)fb_lds_bytes(fb.net[0]);
    const int stage = lds + fb_head_lds(head) <= FB_LDS_LIMIT ? 1 : 0;      // no room: the head reads its targets from memory
    fb_head_stage(head, stage);
    if (stage) lds += fb_head_lds(head);
    auto one = [&](auto g1, auto xb16) -> int32_t {                // one kernel: first hidden width 256 * g1, input form xb16
        const auto kernel = fb_head_kernel<Head, decltype(g1)::value, decltype(xb16)::value, GA>();
        const int32_t rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), lds, fb_head_name(head));
        if (rc) return rc;
        hipLaunchKernelGGL(kernel, dim3(tiles), dim3(1024), lds, s, fb, fl, head);
        return HGYM_OK;
    };
    auto both = [&](auto g1) { return shadow ? one(g1, std::true_type()) : one(g1, std::false_type()); };      // runtime `shadow` -> XB16
    const int g1 = fb.net[0].layer[0].NB / 16;         // first hidden width 256 / 512 / 768
    if (g1 == 1) return both(std::integral_constant<int, 1>());
    if (g1 == 2) return both(std::integral_constant<int, 2>());
    if (g1 == 3) return both(std::integral_constant<int, 3>());
    return HGYM_E_UNSUPPORTED;
}
extern template int32_t launch_mlp_fb_head<false, FbMirror>(const FwdArgs&, const FbLoss&, const FbMirror&, bool, int, hipStream_t);
extern template int32_t launch_mlp_fb_head<true, FbMirror>(const FwdArgs&, const FbLoss&, const FbMirror&, bool, int, hipStream_t);
extern template int32_t launch_mlp_fb_head<false, FbSmooth>(const FwdArgs&, const FbLoss&, const FbSmooth&, bool, int, hipStream_t);
extern template int32_t launch_mlp_fb_head<true, FbSmooth>(const FwdArgs&, const FbLoss&, const FbSmooth&, bool, int, hipStream_t);
extern template int32_t launch_mlp_fb_head<false, FbMirrorSmooth>(const FwdArgs&, const FbLoss&, const FbMirrorSmooth&, bool, int, hipStream_t);
extern template int32_t launch_mlp_fb_head<true, FbMirrorSmooth>(const FwdArgs&, const FbLoss&, const FbMirrorSmooth&, bool, int, hipStream_t);
extern template int32_t launch_mlp_fb_head<false, FbGuide>(const FwdArgs&, const FbLoss&, const FbGuide&, bool, int, hipStream_t);
extern template int32_t launch_mlp_fb_head<true, FbGuide>(const FwdArgs&, const FbLoss&, const FbGuide&, bool, int, hipStream_t);
extern template int32_t launch_mlp_fb_head<false, FbBC>(const FwdArgs&, const FbLoss&, const FbBC&, bool, int, hipStream_t);
extern template int32_t launch_mlp_fb_head<true, FbBC>(const FwdArgs&, const FbLoss&, const FbBC&, bool, int, hipStream_t);

// ================================================================================================ per-minibatch loss scalars
// Sums the per-tile loss partials of a minibatch ([nblocks][32], mlp_fb_kernel / ppo_loss_kernel) into opt_state and writes the
// gradients that are plain column sums: std, the two head biases (fused path), the KL slot behind the flat gradient.
// One workgroup of 256 or 512 threads -- its own launch (ppo_scalars_kernel) or, on the fused path, one extra workgroup of the
// weight-gradient launch that follows the loss anyway (dw_kernel_rs: DwArgs::scal_bid).  The summation order does not depend on the
// thread count (16 interleaved partial sums per quantity, combined in a fixed order).
struct ScalArgs {
    int nblocks, B, A, aux_No;
    const float* partials;
    float* grads_std;
    float* grads_bmu;      // may be null (generic path: the head bias gradients come from the GEMMs)
    float* grads_bv;
    float* kl_slot;
    double* opt;
    double beta1, beta2;   // Adam's: beta^t of the step this gradient will be applied in is left in opt[HGYM_OPT_PROLOGUE_STEP .. HGYM_OPT_BETA2_POW] (below)
    // hgym_ppo_apply's single-thread prologue (adaptive-KL learning rate, Adam step count, bias corrections) done HERE, beside the
    // weight-gradient launch, when the caller has promised that exactly this gradient is applied next on one rank
    // (HgymPPOConfig.grad_norm_ready): it needs nothing but the minibatch KL this block has just formed, and as a launch of its own it
    // sat alone on the critical path between the slab sum and Adam (4.7 us + a launch boundary, eight times per iteration)
    int do_prologue, adaptive_lr;
    float desired_kl;
    double lr_min, lr_max;
    int group;             // 0 / 1: `partials` holds one row per loss workgroup; 4: one row per 16-row block (mlp_fb2_kernel), four
                           // consecutive rows are added first, ((p0 + p1) + p2) + p3 in fp32 -- the sum mlp_fb_kernel's 64-row tile forms
                           // over its four head waves -- and nblocks counts those groups
    const float* sigma;    // HGYM_STD_LOG: the derived sigma block -- the std gradient leaves as d/d(log sigma) = d/d(sigma) * sigma; null: as it is
    double* mirror_sums;   // the mirror loss (HgymBatch.mirror_sums): [0] += the minibatch's MSE, [1] += 1; null: off
};
// ppo.py:140-145, the one copy of the rule (ppo_scalars_block here, apply_prologue in hgym_net.hip).  The reference compares the fp32
// 0-dim tensor kl_mean with python floats, which torch rounds to fp32: the comparisons are fp32 ones against float32(desired_kl * 2) and
// float32(desired_kl / 2) -- 2 * desired_kl and desired_kl / 2 of the fp32 field, exactly -- while the learning rate is a python double.
__device__ __forceinline__ double adapt_lr(double lr, float kl, float desired_kl, double lr_min, double lr_max) {
    if (kl > desired_kl * 2.0f) return fmax(lr_min, lr / 1.5);
    if (kl < desired_kl * 0.5f && kl > 0.0f) return fmin(lr_max, lr * 1.5);
    return lr;
}
// The "prologue done, not applied yet" marker (ppo_scalars_block below, apply_prologue / adam_kernel in hgym_net.hip).  A macro: as an
// inlined function the same expression compiles to different code in ppo_scalars_block and apply_prologue.
#define PROLOGUE_PENDING(opt) ((opt)[HGYM_OPT_PROLOGUE_STEP] == (opt)[HGYM_OPT_STEP] && (opt)[HGYM_OPT_STEP] > 0.0)
__device__ __forceinline__ void ppo_scalars_block(const ScalArgs& a, int tid, int nthreads) {
    __shared__ double red[16][LOSS_PARTIALS + 1];
    // beta1^t, beta2^t for hgym_ppo_apply's prologue: two double-precision pow() are ~6 us in that single-thread kernel, on the
    // minibatch's critical path; here they run on two lanes of the last wavefront beside a launch that takes 170 us anyway.  Keyed
    // by t (opt[PROLOGUE_STEP]): the prologue recomputes them if the step count is not the one assumed here.
    // opt[PROLOGUE_STEP] is also the "prologue done, not applied yet" marker (PROLOGUE_PENDING): == opt[STEP] (> 0) after a prologue taken here or in apply_prologue_kernel,
    // -1 once adam_kernel has applied the step.  A second gradient call before the apply finds the marker set and leaves the step's
    // learning-rate decision, step count and powers alone (the update then is the reference's: one optimiser step per apply).
    if (tid >= nthreads - 2 && !PROLOGUE_PENDING(a.opt)) {
        const double t = a.opt[HGYM_OPT_STEP] + 1.0;
        const double pw = pow(tid == nthreads - 2 ? a.beta1 : a.beta2, t);
        a.opt[tid == nthreads - 2 ? HGYM_OPT_BETA1_POW : HGYM_OPT_BETA2_POW] = pw;
        if (tid == nthreads - 2) a.opt[HGYM_OPT_PROLOGUE_STEP] = t;
    }
    const float* __restrict__ partials = a.partials;
    const int nblocks = a.nblocks, B = a.B, A = a.A;
    const int k = tid & (LOSS_PARTIALS - 1);
    for (int part = tid / LOSS_PARTIALS; part < 16; part += nthreads / LOSS_PARTIALS) {     // 16 partial sums per quantity
        // four independent partial sums (combined in a fixed order): a single dependent chain of nblocks / 16 loads was
        // latency-bound once the fused forward + backward kernel started handing in one partial row per 64-row tile (960 rows)
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        int b = part;
        if (a.group == 4) {
            auto ld = [&](int g) -> float {
                const float* p = partials + (int64_t)g * 4 * LOSS_PARTIALS + k;
                const float p0 = p[0], p1 = p[LOSS_PARTIALS], p2 = p[2 * LOSS_PARTIALS], p3 = p[3 * LOSS_PARTIALS];
                return ((p0 + p1) + p2) + p3;
            };
            for (; b + 48 < nblocks; b += 64) {
                const float v0 = ld(b), v1 = ld(b + 16), v2 = ld(b + 32), v3 = ld(b + 48);
                s0 += (double)v0; s1 += (double)v1; s2 += (double)v2; s3 += (double)v3;
            }
            for (; b < nblocks; b += 16) s0 += (double)ld(b);
        } else {
            for (; b + 48 < nblocks; b += 64) {
                const float v0 = partials[(int64_t)b * LOSS_PARTIALS + k], v1 = partials[(int64_t)(b + 16) * LOSS_PARTIALS + k];
                const float v2 = partials[(int64_t)(b + 32) * LOSS_PARTIALS + k], v3 = partials[(int64_t)(b + 48) * LOSS_PARTIALS + k];
                s0 += (double)v0; s1 += (double)v1; s2 += (double)v2; s3 += (double)v3;
            }
            for (; b < nblocks; b += 16) s0 += (double)partials[(int64_t)b * LOSS_PARTIALS + k];
        }
        red[part][k] = (s0 + s1) + (s2 + s3);
    }
    __syncthreads();
    if (tid < LOSS_PARTIALS) {
        double t = 0.0;
        for (int p = 0; p < 16; ++p) t += red[p][tid];
        const int q = tid;
        double* __restrict__ opt = a.opt;
        if (q == LP_SURROGATE) opt[HGYM_OPT_SURROGATE_SUM] += t / B;
        if (q == LP_VALUE) opt[HGYM_OPT_VALUE_SUM] += t / B;
        if (q == LP_ENTROPY) opt[HGYM_OPT_ENTROPY_SUM] += t / B;
        if (q == LP_KL) {
            const float kl = (float)(t / B);  // the reference's kl_mean is an fp32 tensor: the decision, here and in apply_prologue, is taken on it
            opt[HGYM_OPT_KL_SUM] += t / B;
            opt[HGYM_OPT_KL_LAST] = (double)kl;
            opt[HGYM_OPT_MINIBATCHES] += 1.0;
            opt[HGYM_OPT_GRAD_SQNORM] = 0.0;  // squared gradient norm: accumulated by reduce_slabs_kernel later in this call
            a.kl_slot[0] = kl;                // grads[P]: travels with the gradient in the ranks' one all-reduce
            if (a.do_prologue && !PROLOGUE_PENDING(opt)) {      // apply_prologue_kernel's arithmetic (hgym_net.hip), one rank: ppo.py:140-148
                double lr = opt[HGYM_OPT_LR];
                if (a.adaptive_lr) {
                    lr = adapt_lr(lr, kl, a.desired_kl, a.lr_min, a.lr_max);
                    opt[HGYM_OPT_LR] = lr;
                }
                const double ts = opt[HGYM_OPT_STEP] + 1.0;           // (= opt[PROLOGUE_STEP]: the two lanes above prepared beta^ts before the barrier)
                opt[HGYM_OPT_STEP] = ts;
                const double bc1 = 1.0 - opt[HGYM_OPT_BETA1_POW], bc2 = 1.0 - opt[HGYM_OPT_BETA2_POW];
                opt[HGYM_OPT_STEP_SIZE] = (double)(float)(lr / bc1);      // step size
                opt[HGYM_OPT_SQRT_BC2] = (double)(float)sqrt(bc2);
            }
        }
        if (q >= LP_DSTD && q < LP_DBIAS_MU && q - LP_DSTD < A) {
            // (log mode: the sum rounded to fp32 as ever, then ONE fp32 product -- the chain rule of sigma = exp(log sigma); in place before
            // any pass squares the gradient, so the clip norm is that of the log-std gradient)
            const float g = (float)t;
            a.grads_std[q - LP_DSTD] = a.sigma ? __fmul_rn(g, a.sigma[q - LP_DSTD]) : g;
        }
        if (q >= LP_DBIAS_MU && q < LP_DBIAS_V && q - LP_DBIAS_MU < A && a.grads_bmu) a.grads_bmu[q - LP_DBIAS_MU] = (float)t;
        if (q == LP_DBIAS_V && a.grads_bv) a.grads_bv[0] = (float)t;
        if (q == LP_AUX && a.aux_No > 0) opt[HGYM_OPT_AUX_SUM] += t / ((double)B * (double)a.aux_No);    // auxiliary head's MSE (the fused kernel's third grid row)
        if (q == LP_MIRROR && a.mirror_sums) {      // the mirror loss's MSE: the tile partials in the fixed order of every other sum
            a.mirror_sums[0] += t / ((double)B * (double)A);
            a.mirror_sums[1] += 1.0;
        }
    }
}

// ================================================================================================ weight gradients
// dW[n][k] = sum_m Z[m][n] * X[m][k]  (Z = dZ_l, X = layer input): tiles of 128 dZ columns x 256 input columns, eight wavefronts
// (64 x 64 each), contraction split over blockIdx.y.
//
// How the kernel got its shape (all on B = 61 440, one box, profiles/r03_dw_ablation.txt):
//  * Operand transport: every wave keeps DW_RS stages of its three 1-KiB pieces in registers (global_load_dwordx4) and passes one
//    stage per step to the LDS ring with ds_write_b128; fragments are read with the transpose read.  (A first version DMA'd the
//    pieces straight into LDS with global_load_lds: a piece costs the issuing wave 60-185 cycles (MI355X_MICROARCH.md, LDS-DMA
//    issue cost) next to 20 MFMAs = 320 cycles, so the DMA issue set the pace -- 272 us per launch against 183 us.)
//  * Round 2's kernel (128 x 128 tiles, four waves, two workgroups per CU, 189 us) took the same time with its LDS traffic
//    (177.9 us) or three quarters of its MFMAs (186.1 us) removed, and 135 us when every load hit a page of zeros: the pace is set
//    by the CU's fill path -- 16 KiB per 32-row step per tile, two tiles per CU -- and neither by MFMA nor LDS; not by HBM either:
//    a quarter of the rows, written microseconds earlier and still in the Infinity Cache, is no faster per row, and register rings
//    of 2..5 stages all measure the same.  A 128 x 256 tile moves 24 KiB per step for twice the products -- three quarters of the
//    bytes per MFMA through L1 -- and 32 tiles x 8 splits is exactly one workgroup per CU: 189 -> 180 us.
//  * On L1-resident operands, removing the LDS reads, the LDS writes or three quarters of the MFMAs each saved its own 20-30 us of
//    the 135: a sum, not a maximum -- the waves leave every barrier in the same phase, two MFMA streams queue at each matrix
//    pipe and then nobody uses it.  Hence the two wave groups half a step apart (below): 180 -> 174 us (zero-page floor 133 -> 120).
//  * What remains above the floor is the fill path itself: +29 us when the operands come from L2 (the same two row blocks over and
//    over), +24 us more from HBM.
constexpr int DW_THREADS = 512;
constexpr int DW_Z_BYTES = 8192;           // 32 rows x 8 Z blocks x 512 B
constexpr int DW_STAGE_BYTES = 24576;      // + 32 rows x 16 X blocks
constexpr int DW_LDS_STAGES = 3;
constexpr int DW_TILE_N = 128, DW_TILE_K = 256;
constexpr int DW_MAX_PRODUCTS = 12;        // actor + critic + auxiliary head, four layers each

struct DwProduct {
    const __bf16* Z;      // block layout, CBz column blocks per row block
    const __bf16* X;      // block layout, CBx -- or, with gidx, the row-major bf16 shadow the rows are gathered from
    const int64_t* gidx;  // non-null: batch row m of X is row gidx[m] of the shadow (leading dimension ldg elements, CBx = ldg / 16):
                          // a first-layer product whose operand was never copied (mlp_fb_kernel<XB16>)
    int64_t ldg;
    int CBz, CBx;
    int N, K;             // valid rows / cols of dW (row-major, leading dimension K)
    int64_t w_off;        // offset of dW in a slab (floats)
    int64_t b_off;        // offset of the bias gradient (column sums of Z), -1: none
    int tiles_n, tiles_k, tile0;
};

struct DwArgs {
    DwProduct p[DW_MAX_PRODUCTS];
    int np;
    int total_tiles;
    int splits;
    int steps_total;       // row blocks of 32 over the (padded) batch
    int steps_per_split;
    float* slabs;
    int64_t slab_stride;   // floats
    const char* zeros;     // 4 KiB of zeros (workspace): source of the stages past the end of a split
    int B;                 // valid batch rows (gathered products clamp their row indices to it)
    int scal_bid;          // >= 0: this workgroup sums the minibatch's loss partials instead (ppo_scalars_block); -1: none
    ScalArgs sc;
};

__device__ __forceinline__ u32x4 tr_frag(const char* p0, const char* p1) {
    typedef s16x4 __attribute__((address_space(3)))* lds_p;
    const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(const_cast<char*>(p0)));
    const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(const_cast<char*>(p1)));
    struct { s16x4 a, b; } pr = {a, b};
    return __builtin_bit_cast(u32x4, pr);
}

template <int DW_RS>      // register stages in flight per wave
__global__ __launch_bounds__(DW_THREADS, 1) void dw_kernel_rs(const DwArgs a) {
    static_assert(DW_RS == 3, "ring indices below: three register stages over three LDS stages, unrolled by six");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;                  // 64-column strip of the X side (4), of the Z side (2)
    const int r = lane & 15, q = lane >> 4;
    const int bid = blockIdx.x;
    if (bid == a.scal_bid) {      // the loss scalars ride in this launch: one workgroup, ~10 us beside 170 us of tiles
        ppo_scalars_block(a.sc, tid, DW_THREADS);
        return;
    }
    // Block -> (tile, split).  Workgroups are dealt round-robin to the 8 XCDs (block b -> XCD b % 8), each with a private
    // 4 MiB L2.  All tiles of one split stream the SAME batch rows, so a split is pinned to one XCD: its 32 tiles run there
    // concurrently and every operand block is fetched from HBM once and re-read from that L2 by the other tiles.
    const int xcd = bid & 7, slot = bid >> 3;
    const int split = xcd + 8 * (slot / a.total_tiles);
    const int tile = slot % a.total_tiles;
    if (split >= a.splits) return;
    int pi = 0;
#pragma unroll
    for (int i = 1; i < DW_MAX_PRODUCTS; ++i)
        if (i < a.np && tile >= a.p[i].tile0) pi = i;
    const DwProduct& P = a.p[pi];
    const int tl = tile - P.tile0;
    const int tn = tl / P.tiles_k, tk = tl - tn * P.tiles_k;
    const int cbz0 = tn * 8, cbx0 = tk * 16;
    const int step0 = split * a.steps_per_split;
    int nsteps = a.steps_total - step0;
    nsteps = nsteps < a.steps_per_split ? nsteps : a.steps_per_split;

    // Wave w moves, of every 32-row stage, row block w & 1 of Z block pair w >> 1 and of X block pairs 2 (w >> 1), 2 (w >> 1) + 1
    // (piece = two adjacent 16 x 16 blocks of one row block, 1 KiB, lane-linear).
    //
    // Addressing: every load is (wave-uniform 64-bit base in SGPRs, advanced by scalar arithmetic) + (32-bit per-lane byte offset),
    // the saddr form of global_load; per-lane 64-bit addresses cost ~50 of a step's 126 instructions.  "Past the end of the split ->
    // the page of zeros" is a scalar select on that base, never a branch around a load (a conditional load makes the compiler's
    // vmcnt conservative), and an OFFSET from the operand's own pointer (a pointer rebuilt from an integer becomes a FLAT access).
    //
    // Gathered X operand (first-layer products on the bf16 shadow, < 4 GiB: FusedPath::grad checks): the lane that holds bytes
    // [16 l, 16 l + 16) of a piece holds row (l & 31) >> 1 of the row block, block l >> 5 of the pair, half l & 1 -- in the row-major
    // shadow that is 16 bytes of row gidx[m].  The 16 row indices of a stage are one 4-byte load per lane (row l & 15, replicated
    // over the wave) issued TWO stages ahead of the stage's data and in front of the data loads issued with it: a wave's loads
    // return in order, so when the index is needed only the younger stages are behind it and the data ring keeps its depth.  Every
    // tile issues the index load (from the zero page when it has nothing to gather): one instruction stream, exact vmcnt.
    const int mbl = __builtin_amdgcn_readfirstlane(wave & 1), pp = __builtin_amdgcn_readfirstlane(wave >> 1);
    const char* zbase = reinterpret_cast<const char*>(P.Z);
    const char* xbase = reinterpret_cast<const char*>(P.X);
    const bool gx = P.gidx != nullptr;
    const unsigned int lofs = lane * 16;
    int cbz = cbz0 + 2 * pp;
    cbz = cbz + 1 < P.CBz ? cbz : P.CBz - 2;                          // surplus pairs: clamped onto valid blocks (results unused)
    const int64_t zofs = ((int64_t)(2 * step0 + mbl) * P.CBz + cbz) * 512;
    const int64_t zstep = (int64_t)2 * P.CBz * 512;                   // bytes per 32-row step
    const unsigned int ldgb = (unsigned int)(P.ldg * 2);
    const int irow = mbl * 16 + (lane & 15);                          // row of the 32-row step whose index this lane fetches
    const int bsrc = ((lane & 31) >> 1) * 4;                          // ds_bpermute address: the lane that holds this lane's row
    unsigned int vb[2];                                               // per-lane constant part of the byte offset
    int64_t xofs[2];                                                  // wave-uniform part: the piece's offset in a linear operand
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        int cb = cbx0 + 2 * (2 * pp + j);
        cb = cb + 1 < P.CBx ? cb : P.CBx - 2;
        const unsigned int gcol = (unsigned int)(((cb + (lane >> 5)) * 16 + (lane & 1) * 8) * 2);
        vb[j] = gx ? gcol : lofs;
        xofs[j] = gx ? 0 : ((int64_t)(2 * step0 + mbl) * P.CBx + cb) * 512;
    }
    const int64_t xstep = gx ? 0 : (int64_t)2 * P.CBx * 512;
    const int64_t zdz = a.zeros - zbase, zdx = a.zeros - xbase;
    const char* ibase = gx ? reinterpret_cast<const char*>(P.gidx) : a.zeros;
    const int mg0 = gx ? -1 : 0;
    auto load_idx = [&](int t) -> int {
        int mrow = (step0 + (t < nsteps ? t : nsteps - 1)) * 32 + irow;
        mrow = mrow < a.B ? mrow : a.B - 1;
        // the low word only (indices are < 2^31): the dead upper half of an 8-byte load is a register the allocator hands out
        // again at once, and overwriting it has to wait for the load -- i.e. for every older load of the ring
        return *reinterpret_cast<const int*>(ibase + ((unsigned int)((mrow & mg0) | ((lane & 15) & ~mg0)) << 3));
    };
    // index ring: slot t % 3 holds the indices of stage t (a compile-time slot in the unrolled loop: rotating two registers
    // instead costs a move of a just-loaded value, i.e. a wait that drains the data ring once per revolution)
    int GI[3];
    GI[0] = load_idx(0);
    GI[1] = load_idx(1);
    u32x4 R[DW_RS][3];
    auto load = [&](int t, int slot3, u32x4 (&rr)[3]) {               // slot3 == t % 3
        const bool in = t < nsteps;                                   // wave-uniform: scalar selects below
        GI[(slot3 + 2) % 3] = load_idx(t + 2);                        // issued BEFORE this stage's data
        const unsigned int rmask = (gx && in) ? 0xffffffffu : 0u;
        const unsigned int rterm = ((unsigned int)__builtin_amdgcn_ds_bpermute(bsrc, GI[slot3]) * ldgb) & rmask;
        const int64_t m = in ? -1 : 0;                                // (integer masks: a `?:` on the pointer becomes a branch)
        rr[0] = *reinterpret_cast<const u32x4*>(zbase + (((zofs + (int64_t)t * zstep) & m) | (zdz & ~m)) + lofs);
#pragma unroll
        for (int j = 0; j < 2; ++j)
            rr[1 + j] = *reinterpret_cast<const u32x4*>(xbase + (((xofs[j] + (int64_t)t * xstep) & m) | (zdx & ~m)) + (vb[j] + rterm));
    };
    // LDS stage: [row block][8 Z blocks][512 B], then [row block][16 X blocks][512 B]
    auto store = [&](int buf, const u32x4 (&rr)[3]) {
        char* dz = smem + buf * DW_STAGE_BYTES + mbl * 4096 + pp * 1024 + lane * 16;
        char* dx = smem + buf * DW_STAGE_BYTES + DW_Z_BYTES + mbl * 8192 + pp * 2048 + lane * 16;
        *reinterpret_cast<u32x4*>(dz) = rr[0];
        *reinterpret_cast<u32x4*>(dx) = rr[1];
        *reinterpret_cast<u32x4*>(dx + 1024) = rr[2];
    };

    f32x4 acc[4][4];
    f32x4 accb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        accb[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const bool do_bias = (P.b_off >= 0) && tk == 0 && wi == 0;
    const u32x4 ones = {0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u};
    auto frags = [&](int stage, u32x4 (&xa)[4], u32x4 (&zb)[4]) {
        const char* st = smem + stage * DW_STAGE_BYTES;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const char* px = st + DW_Z_BYTES + (wi * 4 + i) * 512 + lane * 8;
            xa[i] = tr_frag(px, px + 8192);
            const char* pz = st + (wj * 4 + i) * 512 + lane * 8;
            zb[i] = tr_frag(pz, pz + 4096);
        }
    };
    auto mfmas = [&](const u32x4 (&xa)[4], const u32x4 (&zb)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) mma_frag<__bf16>(xa[i], zb[jj], acc[i][jj]);
        if (do_bias) {      // column sums of Z (measured: making every tile issue them, to keep a split's tiles in step, changes nothing)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) mma_frag<__bf16>(ones, zb[jj], accb[jj]);
        }
    };

    // Pipeline.  The LDS ring holds stages t, t + 1 (read) and t + 2 (being written), the register ring stages t + 2 .. t + 4; the
    // MFMAs of step t run on fragments read during step t - 1.  A step is two half-steps with a barrier after each, and the
    // wavefronts work in two groups half a step apart: while waves 0-3 (one per SIMD) issue the MFMAs of a step, waves 4-7 --
    // their SIMD partners -- move data (global loads of stage t + 4, LDS writes of stage t + 2, transpose reads of step t + 1),
    // and vice versa.  The lagging group enters one barrier late and the leading group leaves one barrier late: every wave
    // executes the same number of barriers.  Stage t + 2 is written in half-steps 2t + 1 (leading) and 2t + 2 (lagging) and first
    // read in half-step 2t + 3; its buffer was last read (stage t - 1) in half-step 2t - 2.  The steady-state loop is branch-free
    // -- stages past the end of the split come from the page of zeros and add nothing.
    u32x4 XA[2][4], ZB[2][4];
#pragma unroll
    for (int j = 0; j < DW_RS; ++j) load(j, j % 3, R[j]);
    store(0, R[0]);
    load(DW_RS, DW_RS % 3, R[0]);
    store(1, R[1]);
    __syncthreads();
    frags(0, XA[0], ZB[0]);
    const int np = (nsteps + 5) / 6 * 6;
    const int lagw = __builtin_amdgcn_readfirstlane(wave >> 2);
    if (lagw) __builtin_amdgcn_s_barrier();
    for (int t0 = 0; t0 < np; t0 += 6) {
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int t = t0 + j;
            __builtin_amdgcn_s_setprio(1);
            mfmas(XA[j & 1], ZB[j & 1]);
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();
            load(t + 1 + DW_RS, (j + 1 + DW_RS) % 3, R[(j + 1) % DW_RS]);      // that slot held stage t + 1: in LDS since step t - 1
            __builtin_amdgcn_sched_barrier(0);
            store((j + 2) % 3, R[(j + 2) % DW_RS]);                            // stage t + 2, loaded two steps ago
            frags((j + 1) % 3, XA[(j + 1) & 1], ZB[(j + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();
        }
    }
    if (!lagw) __builtin_amdgcn_s_barrier();

    // lane holds dW[n = .. + r][k = .. + 4q + e]
    float* __restrict__ slab = a.slabs + (int64_t)split * a.slab_stride;
    float* __restrict__ out = slab + P.w_off;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int nn = (cbz0 + wj * 4 + j) * 16 + r;
        if (nn >= P.N) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int kk = (cbx0 + wi * 4 + i) * 16 + 4 * q;
            float* p = out + (int64_t)nn * P.K + kk;
            if (kk + 3 < P.K) {
                F4 v = {{acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]}};
                *reinterpret_cast<F4*>(p) = v;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (kk + e < P.K) p[e] = acc[i][j][e];
            }
        }
        if (do_bias && q == 0) slab[P.b_off + nn] = accb[j][0];
    }
}

}  // namespace hgym

#ifdef HGYM_TU_CONTRACT_OFF
#pragma clang fp contract(off)
#endif
