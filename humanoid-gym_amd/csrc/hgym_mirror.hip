// hgym_mirror.hip -- hgym_mirror_rows: the left-right mirrored copy of stored rollout rows (PPO.symmetry).
//
// dst[m][c] = bits(src[m][src_col[c]]) ^ (sign[c] < 0 ? sign bit : 0) for c < width, +0 for width <= c < zero_to.  A pure stream: every
// byte is read once and written once.  A workgroup stages a block of whole source rows in LDS with coalesced loads, then writes the
// destination rows in order, reading LDS through the column table -- the permutation costs LDS reads, never an uncoalesced access.
// Rows are only element-aligned in general (705 floats = 2820 bytes), so every contiguous span -- a row, or the whole row block when
// ld == width -- is cut into an unaligned head, a body of 16-byte accesses and a tail; an aligned layout (the bf16 shadows) has no head.
#include "hgym_common.hpp"

namespace hgym {

constexpr int MIRROR_THREADS = 256;
constexpr int MIRROR_STAGE_BYTES = 32 * 1024;     // staged rows of one block (with the table: 40 KiB at most, four blocks per CU)
constexpr int MIRROR_MAX_ROWS = 256;              // ... and at most this many rows, so that spans stay far inside 32-bit indices
constexpr int MIRROR_MAX_BLOCKS = 2048;           // blocks loop over row blocks: the table is loaded once per block, not per row block
constexpr uint32_t MIRROR_NEG = 0x80000000u;      // table entry: source column | MIRROR_NEG where the sign bit is inverted

// Item k of a span of `len` elements starting at address `base`: k = 0 is the head (the elements in front of the first 16-byte boundary),
// k = 1 .. nbody the aligned 16-byte pieces, k = nbody + 1 the tail; larger k: nothing.  -> first element e0 and the count n (0 .. V).
template <typename E>
__device__ __forceinline__ void span_item(uintptr_t base, int len, int k, int& e0, int& n) {
    constexpr int V = 16 / (int)sizeof(E);
    const int head = min(len, (int)(((0 - base) & 15) / sizeof(E)));
    const int nbody = (len - head) / V;
    if (k == 0) {
        e0 = 0;
        n = head;
    } else if (k <= nbody) {
        e0 = head + (k - 1) * V;
        n = V;
    } else {
        e0 = head + nbody * V;
        n = k == nbody + 1 ? len - e0 : 0;
    }
}

template <typename E>
union Piece {
    uint4 q;
    E e[16 / sizeof(E)];
};

// E: the element's bit pattern (uint32_t: fp32, uint16_t: bf16).  rows: rows per block (the host's choice: rows * width * sizeof(E) fits
// the staging area).  zt = zero_to.  Dynamic LDS: [width] uint32 table | rows * width elements.
template <typename E>
__global__ __launch_bounds__(MIRROR_THREADS) void mirror_rows_kernel(int64_t M, int width, int zt, int rows, const int32_t* __restrict__ src_col,
                                                                      const float* __restrict__ sign, const E* __restrict__ src, int64_t ld_src,
                                                                      E* __restrict__ dst, int64_t ld_dst) {
    constexpr int V = 16 / (int)sizeof(E);
    constexpr E SIGN = (E)((E)1 << (8 * sizeof(E) - 1));
    extern __shared__ __attribute__((aligned(16))) uint32_t mirror_lds[];
    uint32_t* tab = mirror_lds;
    E* stage = (E*)(mirror_lds + ((width + 3) & ~3));
    const int tid = threadIdx.x;
    for (int c = tid; c < width; c += MIRROR_THREADS) {
        // the library cannot know what the caller's table holds: a column outside the row reads the row's last column, never other memory
        const uint32_t sc = (uint32_t)src_col[c];
        tab[c] = (sc < (uint32_t)width ? sc : (uint32_t)(width - 1)) | (sign[c] < 0.0f ? MIRROR_NEG : 0u);
    }
    const bool flat_s = ld_src == width, flat_d = ld_dst == zt;       // rows back to back: the whole row block is one span
    const int64_t nblk = (M + rows - 1) / rows;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t m0 = blk * rows;
        const int nr = (int)min((int64_t)rows, M - m0);
        __syncthreads();      // the table is there; the previous row block's stores have read the staging area
        {   // global -> LDS, row-major [nr][width]
            const int len = flat_s ? nr * width : width, nspan = flat_s ? 1 : nr;
            const uint32_t per = (uint32_t)(len / V + 2);
            for (uint32_t i = tid; i < per * (uint32_t)nspan; i += MIRROR_THREADS) {
                const uint32_t s = flat_s ? 0u : i / per;
                const E* p = src + (m0 + s) * ld_src;
                int e0, n;
                span_item<E>((uintptr_t)p, len, (int)(i - s * per), e0, n);
                E* l = stage + (size_t)s * width + e0;
                if (n == V) {
                    Piece<E> u;
                    u.q = *reinterpret_cast<const uint4*>(p + e0);
#pragma unroll
                    for (int j = 0; j < V; ++j) l[j] = u.e[j];
                } else {
                    for (int j = 0; j < n; ++j) l[j] = p[e0 + j];
                }
            }
        }
        __syncthreads();
        {   // LDS -> global through the table, destination rows in order ([0, zt) of each; pads written as +0)
            const int len = flat_d ? nr * zt : zt, nspan = flat_d ? 1 : nr;
            const uint32_t per = (uint32_t)(len / V + 2);
            for (uint32_t i = tid; i < per * (uint32_t)nspan; i += MIRROR_THREADS) {
                const uint32_t s = flat_d ? 0u : i / per;
                E* p = dst + (m0 + s) * ld_dst;
                int e0, n;
                span_item<E>((uintptr_t)p, len, (int)(i - s * per), e0, n);
                if (n == 0) continue;
                int r = flat_d ? e0 / zt : (int)s;
                int c = flat_d ? e0 - r * zt : e0;
                Piece<E> u;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    E v = 0;
                    if (j < n) {
                        if (c < width) {
                            const uint32_t t = tab[c];
                            v = stage[(size_t)r * width + (t & 0xFFFFu)] ^ ((t & MIRROR_NEG) ? SIGN : (E)0);
                        }
                        if (++c == zt) {
                            c = 0;
                            ++r;
                        }
                    }
                    u.e[j] = v;
                }
                if (n == V) {
                    *reinterpret_cast<uint4*>(p + e0) = u.q;
                } else {
#pragma unroll
                    for (int j = 0; j < V; ++j)
                        if (j < n) p[e0 + j] = u.e[j];
                }
            }
        }
    }
}

template <typename E>
static int32_t launch_mirror(int64_t M, int width, int zt, const int32_t* src_col, const float* sign, const void* src, int64_t ld_src, void* dst,
                             int64_t ld_dst, hipStream_t s) {
    int rows = MIRROR_STAGE_BYTES / (width * (int)sizeof(E));
    rows = rows < 1 ? 1 : rows > MIRROR_MAX_ROWS ? MIRROR_MAX_ROWS : rows;
    const size_t lds = (size_t)((width + 3) & ~3) * 4 + (size_t)rows * width * sizeof(E);
    const int64_t nblk = (M + rows - 1) / rows;
    const int blocks = (int)(nblk < MIRROR_MAX_BLOCKS ? nblk : MIRROR_MAX_BLOCKS);
    hipLaunchKernelGGL(mirror_rows_kernel<E>, dim3(blocks), dim3(MIRROR_THREADS), lds, s, M, width, zt, rows, src_col, sign, (const E*)src, ld_src,
                       (E*)dst, ld_dst);
    HG_CHECK_LAUNCH("mirror_rows_kernel");
    return HGYM_OK;
}

}  // namespace hgym

using namespace hgym;

extern "C" {

int32_t hgym_mirror_rows(int64_t M, int32_t width, const int32_t* src_col, const float* sign, const void* src, int64_t ld_src, void* dst,
                         int64_t ld_dst, int32_t zero_to, int32_t dtype, void* stream) {
    HG_REQUIRE(src_col && sign && src && dst, HGYM_E_BADARG, "null pointer");
    HG_REQUIRE(dtype == HGYM_F32 || dtype == HGYM_BF16, HGYM_E_BADARG, "dtype=%d", dtype);
    HG_REQUIRE(M >= 0 && width >= 1, HGYM_E_BADARG, "M=%lld width=%d", (long long)M, width);
    HG_REQUIRE(ld_src >= width && ld_dst >= width, HGYM_E_BADARG, "ld_src=%lld ld_dst=%lld width=%d", (long long)ld_src, (long long)ld_dst, width);
    HG_REQUIRE(zero_to >= width && zero_to <= ld_dst, HGYM_E_BADARG, "zero_to=%d outside [width=%d, ld_dst=%lld]", zero_to, width, (long long)ld_dst);
    const int64_t es = dtype == HGYM_F32 ? 4 : 2;
    HG_REQUIRE(((uintptr_t)src % es) == 0 && ((uintptr_t)dst % es) == 0, HGYM_E_BADARG, "rows are not aligned to their element size");
    HG_REQUIRE(zero_to <= HGYM_MIRROR_MAX_WIDTH, HGYM_E_UNSUPPORTED, "width=%d zero_to=%d beyond HGYM_MIRROR_MAX_WIDTH=%d", width, zero_to,
               HGYM_MIRROR_MAX_WIDTH);
    // (byte offsets stay inside 63 bits: M * ld * 4 < 2^62)
    HG_REQUIRE(M <= ((int64_t)1 << 40) && ld_src <= (1 << 20) && ld_dst <= (1 << 20), HGYM_E_UNSUPPORTED, "M=%lld ld_src=%lld ld_dst=%lld", (long long)M,
               (long long)ld_src, (long long)ld_dst);
    if (M > 0) {
        const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)(((M - 1) * ld_src + width) * es);
        const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)(((M - 1) * ld_dst + zero_to) * es);
        HG_REQUIRE(s1 <= d0 || d1 <= s0, HGYM_E_BADARG, "src and dst overlap");
    }
    if (M == 0) return HGYM_OK;
    return dtype == HGYM_F32 ? launch_mirror<uint32_t>(M, width, zero_to, src_col, sign, src, ld_src, dst, ld_dst, (hipStream_t)stream)
                             : launch_mirror<uint16_t>(M, width, zero_to, src_col, sign, src, ld_src, dst, ld_dst, (hipStream_t)stream);
}

}  // extern "C"
