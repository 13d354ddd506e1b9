// Layout kernels of Ulysses sequence parallelism (attention_backend "usp", batch 1): the all-to-all send / receive images of the
// draft attention's q | k | v and output, HBM-bound, 16-byte accesses per lane.
//
// Replaces, for the EAGLE3 USP path of the reference:
//   specforge/modeling/draft/llama3_eagle.py:1363-1505  LlamaUSPFlashAttention (RoPE at the global positions, the seq -> head
//                                                       all-to-all of q / k / v and the head -> seq all-to-all of the output)
// plus the autograd backward of each.
//
// Layouts (sp ranks, `chunk` token rows per rank, gq = nh / sp, gk = nkv / sp query / key-value heads per rank):
//   token rows   [chunk, (nh + 2 nkv) hd]            the fused QKV GEMM output of one TTT step (q heads | k heads | v heads)
//   send / recv  [sp][chunk][(gq + 2 gk) hd]         block j: the heads of rank j's group (its gq q | gk k | gk v heads)
// With batch 1, what rank r receives -- block j = rank j's tokens, rank r's heads -- IS the head-sharded [sp chunk, (gq + 2 gk) hd]
// layout the attention kernels read (q / k / v are column ranges of it), at global rows j chunk + t.  The attention output
// [sp chunk, gq hd] is likewise already the send image of the way back; only the token-major side needs a kernel.
#include "sf_api_internal.h"
#include "sf_util.h"

namespace {

inline int ulysses_grid(long units) {
    long g = (units + 255) / 256;
    if (g < 1) g = 1;
    if (g > 256 * 8) g = 256 * 8;
    return (int)g;
}

// One unit = 8 channels of the first half of a head and the matching 8 of its second half (the RoPE pair).
// forward : token rows -> sharded, q / k rotated at position pos_ids[t] + pos_off; the arithmetic of rope_kernel (sf_pointwise.hip)
//           expression for expression, so the result has the bits of sf_rope followed by a permutation
// backward: sharded -> token rows, the transposed rotation (d(q|k) before RoPE), v copied
template <int BWD>
SF_GLOBAL void ulysses_qkv_kernel(const sf_bf16* src, long ld_src, sf_bf16* dst, long ld_dst, int chunk, int nh, int nkv, int hd,
                                  int gq, int gk, const sf_bf16* cos_t, const sf_bf16* sin_t, const long long* pos_ids, int pos_off,
                                  int max_pos) {
    const int half = hd >> 1, upr = half >> 3, nall = nh + 2 * nkv;
    const long per_row = (long)nall * upr, total = (long)chunk * per_row;
    for (long u = (long)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (long)gridDim.x * blockDim.x) {
        const int t = (int)(u / per_row);
        const int rem = (int)(u - (long)t * per_row);
        const int h = rem / upr, jc = (rem - h * upr) * 8;
        int blk, lh;
        bool rot = true;
        if (h < nh) {
            blk = h / gq;
            lh = h - blk * gq;
        } else if (h < nh + nkv) {
            blk = (h - nh) / gk;
            lh = gq + (h - nh) - blk * gk;
        } else {
            blk = (h - nh - nkv) / gk;
            lh = gq + gk + (h - nh - nkv) - blk * gk;
            rot = false;
        }
        const sf_bf16* tokp = src + (long)t * ld_src + (long)h * hd + jc;                         // (forward: read here)
        const long shoff = ((long)blk * chunk + t) * (BWD ? ld_src : ld_dst) + (long)lh * hd + jc;
        const sf_bf16* p1 = BWD ? src + shoff : tokp;
        sf_bf16* q1 = BWD ? dst + (long)t * ld_dst + (long)h * hd + jc : dst + shoff;
        float x1[8], x2[8], o1[8], o2[8];
        SfVec8<sf_bf16>::ld(p1, x1);
        SfVec8<sf_bf16>::ld(p1 + half, x2);
        if (rot) {
            long pos = pos_ids[t] + pos_off;
            if (pos < 0) pos = 0;
            if (pos >= max_pos) pos = max_pos - 1;
            const sf_bf16* cr = cos_t + pos * hd;
            const sf_bf16* sr = sin_t + pos * hd;
            float c1[8], c2[8], s1[8], s2[8];
            SfVec8<sf_bf16>::ld(cr + jc, c1);
            SfVec8<sf_bf16>::ld(cr + half + jc, c2);
            SfVec8<sf_bf16>::ld(sr + jc, s1);
            SfVec8<sf_bf16>::ld(sr + half + jc, s2);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (!BWD) {
                    o1[i] = SfElem<sf_bf16>::rnd(x1[i] * c1[i]) + SfElem<sf_bf16>::rnd(-x2[i] * s1[i]);
                    o2[i] = SfElem<sf_bf16>::rnd(x2[i] * c2[i]) + SfElem<sf_bf16>::rnd(x1[i] * s2[i]);
                } else {
                    o1[i] = x1[i] * c1[i] + x2[i] * s2[i];
                    o2[i] = x2[i] * c2[i] - x1[i] * s1[i];
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                o1[i] = x1[i];
                o2[i] = x2[i];
            }
        }
        SfVec8<sf_bf16>::st(q1, o1);
        SfVec8<sf_bf16>::st(q1 + half, o2);
    }
}

// token-major [chunk, sp w] <-> blocked [sp][chunk][w] (row j chunk + t of the blocked side = block j, token t); 8 columns per unit,
// consecutive units walk the token-major row
template <int TO_TOKENS>
SF_GLOBAL void ulysses_o_kernel(const sf_bf16* src, long ld_src, sf_bf16* dst, long ld_dst, int chunk, int sp, int w) {
    const int w8 = w >> 3;
    const long per_row = (long)sp * w8, total = (long)chunk * per_row;
    for (long u = (long)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (long)gridDim.x * blockDim.x) {
        const int t = (int)(u / per_row);
        const int rem = (int)(u - (long)t * per_row);
        const int j = rem / w8, c = (rem - j * w8) * 8;
        const long tok = (long)t * (TO_TOKENS ? ld_dst : ld_src) + (long)j * w + c;
        const long blk = ((long)j * chunk + t) * (TO_TOKENS ? ld_src : ld_dst) + c;
        *reinterpret_cast<sf_v8s*>(dst + (TO_TOKENS ? tok : blk)) = *reinterpret_cast<const sf_v8s*>(src + (TO_TOKENS ? blk : tok));
    }
}

}  // namespace

extern "C" int sf_ulysses_pack_qkv(const void* src, long ld_src, void* dst, long ld_dst, int chunk, int sp, int nh, int nkv, int hd,
                                   const void* cos_t, const void* sin_t, const long long* pos_ids, int pos_off, int max_pos,
                                   int backward, void* stream) {
    SF_CHECK_ARG(chunk >= 0 && sp >= 1 && nh > 0 && nkv > 0 && nh % sp == 0 && nkv % sp == 0 && nh % nkv == 0,
                 "sf_ulysses_pack_qkv: heads must split evenly over the sp ranks");
    SF_CHECK_ARG(hd % 16 == 0 && max_pos > 0 && ld_src % 8 == 0 && ld_dst % 8 == 0, "sf_ulysses_pack_qkv: bad shape");
    const long wtok = (long)(nh + 2 * nkv) * hd, wsh = wtok / sp;
    SF_CHECK_ARG(backward ? (ld_src >= wsh && ld_dst >= wtok) : (ld_src >= wtok && ld_dst >= wsh),
                 "sf_ulysses_pack_qkv: row stride narrower than the row");
    if (chunk == 0) return 0;
    const long units = (long)chunk * (nh + 2 * nkv) * (hd / 16);
    const int gq = nh / sp, gk = nkv / sp;
    if (backward)
        SF_LAUNCH((ulysses_qkv_kernel<1>), dim3(ulysses_grid(units)), dim3(256), 0, stream, (const sf_bf16*)src, ld_src, (sf_bf16*)dst,
                  ld_dst, chunk, nh, nkv, hd, gq, gk, (const sf_bf16*)cos_t, (const sf_bf16*)sin_t, pos_ids, pos_off, max_pos);
    else
        SF_LAUNCH((ulysses_qkv_kernel<0>), dim3(ulysses_grid(units)), dim3(256), 0, stream, (const sf_bf16*)src, ld_src, (sf_bf16*)dst,
                  ld_dst, chunk, nh, nkv, hd, gq, gk, (const sf_bf16*)cos_t, (const sf_bf16*)sin_t, pos_ids, pos_off, max_pos);
    return sf_check_launch("sf_ulysses_pack_qkv");
}

extern "C" int sf_ulysses_pack_o(const void* src, long ld_src, void* dst, long ld_dst, int chunk, int sp, int w, void* stream) {
    SF_CHECK_ARG(chunk >= 0 && sp >= 1 && w > 0 && w % 8 == 0 && ld_src % 8 == 0 && ld_dst % 8 == 0 && ld_src >= (long)sp * w &&
                 ld_dst >= w, "sf_ulysses_pack_o: bad shape");
    if (chunk == 0) return 0;
    SF_LAUNCH((ulysses_o_kernel<0>), dim3(ulysses_grid((long)chunk * sp * (w / 8))), dim3(256), 0, stream, (const sf_bf16*)src, ld_src,
              (sf_bf16*)dst, ld_dst, chunk, sp, w);
    return sf_check_launch("sf_ulysses_pack_o");
}

extern "C" int sf_ulysses_unpack_o(const void* src, long ld_src, void* dst, long ld_dst, int chunk, int sp, int w, void* stream) {
    SF_CHECK_ARG(chunk >= 0 && sp >= 1 && w > 0 && w % 8 == 0 && ld_src % 8 == 0 && ld_dst % 8 == 0 && ld_dst >= (long)sp * w &&
                 ld_src >= w, "sf_ulysses_unpack_o: bad shape");
    if (chunk == 0) return 0;
    SF_LAUNCH((ulysses_o_kernel<1>), dim3(ulysses_grid((long)chunk * sp * (w / 8))), dim3(256), 0, stream, (const sf_bf16*)src, ld_src,
              (sf_bf16*)dst, ld_dst, chunk, sp, w);
    return sf_check_launch("sf_ulysses_unpack_o");
}
