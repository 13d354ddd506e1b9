// Rank of the target token in one row of draft logits, and the per-row top-k hits built from it.
//
// EAGLE3 drafts are served as top-k trees; the quality signal of the training path (sf_ce_fused: argmax == target) is top-1 only.
// rank = #{ j : z_j > z_t } + #{ j < t : z_j == z_t }   (t = the draft index of the row's target; ties go to the lower index, the rule
// of am_pick in sf_loss.hip and of torch.argmax, so rank == 0 exactly on the rows sf_ce_fused counts as correct).
//
// HBM-bound: one workgroup per row, every logit read once (2 * V bytes per bf16 row), nothing written back to the logits.  Rows
// without a loss mask or whose target has no draft index read nothing at all.
#include "sf_api_internal.h"
#include "sf_util.h"

namespace {

constexpr int TOPK_MAX = 8;
struct TopkThresholds { int k[TOPK_MAX]; };

// Row r (token row rt = row_map ? row_map[r] : r, (b, s) = (rt / S, rt % S)) reads its loss mask and target id at padded index
// b*Spad + s + off: the addressing of ce_fused_kernel.
template <typename T>
SF_GLOBAL void SF_LAUNCH_BOUNDS(256, 2)
topk_rank_kernel(const T* logits, long ld, int rows, int V, int S, int Spad, int off, const int* loss_mask_pad,
                 const long long* tgt_ids_pad, const int* t2d_index, int Vt, const long long* row_map, int J, TopkThresholds kk,
                 int* row_rank, float* row_hit) {
    SF_SHARED int redi[16];
    const int r = (int)blockIdx.x;
    const int rt = row_map ? (int)row_map[r] : r;
    const int b = rt / S, s = rt - b * S;
    const long pr = (long)b * Spad + s + off;
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const int lm = loss_mask_pad[pr];
    // the target's draft index, or -1: no loss mask, an id outside the target vocabulary, an id the draft vocabulary lacks
    int t = -1;
    if (lm != 0) {
        const long long tt = tgt_ids_pad[pr];
        if (t2d_index) {
            if (tt >= 0 && tt < (long long)Vt) t = t2d_index[tt];
        } else if (tt >= 0 && tt < (long long)V) {
            t = (int)tt;
        }
        if (t >= V) t = -1;
    }
    if (t < 0) {    // the sentinel: rank V, no hit at any threshold (workgroup-uniform exit, before any barrier)
        if (tid == 0) {
            if (row_rank) row_rank[r] = V;
            for (int j = 0; j < J; ++j) row_hit[(long)j * rows + r] = 0.f;
        }
        return;
    }
    const T* x = logits + (long)r * ld;
    const float zt = SfElem<T>::ld(x + t);      // one load of a workgroup-uniform address
    const int V8 = V >> 3;
    int gt = 0, eq = 0;
    auto chunk = [&](int c, const SfRaw8<T>& raw) {
        const int below = t - c * 8;            // columns of this chunk in front of the target's
#pragma unroll
        for (int i = 0; i < 8; ++i) gt += raw.at(i) > zt ? 1 : 0;
        if (below > 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) eq += (raw.at(i) == zt && i < below) ? 1 : 0;
        }
    };
    // four 16-byte chunks in flight per lane, as the fused CE streams its rows (for fp32 a chunk is two 16-byte loads)
    constexpr int PU = 4;
    int c = tid;
    for (; c + (PU - 1) * nt < V8; c += PU * nt) {
        SfRaw8<T> raw[PU];
#pragma unroll
        for (int u = 0; u < PU; ++u) raw[u].ld(x + (c + u * nt) * 8);
#pragma unroll
        for (int u = 0; u < PU; ++u) chunk(c + u * nt, raw[u]);
    }
    for (; c < V8; c += nt) {
        SfRaw8<T> raw;
        raw.ld(x + c * 8);
        chunk(c, raw);
    }
    for (int j = V8 * 8 + tid; j < V; j += nt) {    // tail (V % 8)
        const float v = SfElem<T>::ld(x + j);
        gt += v > zt ? 1 : 0;
        eq += (v == zt && j < t) ? 1 : 0;
    }
    for (int m = 32; m >= 1; m >>= 1) {
        gt += sf_shfl_xor(gt, m);
        eq += sf_shfl_xor(eq, m);
    }
    const int w = tid >> 6, nw = nt >> 6;
    if (sf_lane() == 0) { redi[w] = gt; redi[8 + w] = eq; }
    sf_syncthreads();
    if (tid == 0) {
        int rank = 0;
        for (int i = 0; i < nw; ++i) rank += redi[i] + redi[8 + i];
        if (row_rank) row_rank[r] = rank;
        for (int j = 0; j < J; ++j) row_hit[(long)j * rows + r] = rank < kk.k[j] ? (float)lm : 0.f;
    }
}

}  // namespace

extern "C" int sf_topk_rank(const void* logits, int dtype, long ld, int rows, int V, int S, int Spad, int off,
                            const int* loss_mask_pad, const long long* tgt_ids_pad, const int* t2d_index, int Vt,
                            const long long* row_map, int J, const int* kk, int* row_rank, float* row_hit, void* stream) {
    SF_CHECK_ARG(rows >= 0 && V > 0 && S > 0 && Spad >= S && off >= 0 && off + S <= Spad, "sf_topk_rank: bad shape");
    SF_CHECK_ARG(dtype == SF_BF16 || dtype == SF_F32, "sf_topk_rank: dtype");
    SF_CHECK_ARG(J >= 0 && J <= TOPK_MAX && (J == 0 || (kk && row_hit)), "sf_topk_rank: 0 to 8 thresholds, with kk and row_hit");
    SF_CHECK_ARG(ld % 8 == 0 && ld >= V && ((size_t)logits & 15) == 0, "sf_topk_rank: ld must be a multiple of 8 and >= V, logits 16-byte aligned");
    SF_CHECK_ARG(logits && loss_mask_pad && tgt_ids_pad && (row_rank || J > 0), "sf_topk_rank: missing input or no output");
    SF_CHECK_ARG(!t2d_index || Vt > 0, "sf_topk_rank: t2d_index needs its length Vt");
    TopkThresholds th;
    for (int j = 0; j < TOPK_MAX; ++j) th.k[j] = 0;
    for (int j = 0; j < J; ++j) {
        SF_CHECK_ARG(kk[j] >= 1, "sf_topk_rank: thresholds must be positive");
        th.k[j] = kk[j];
    }
    if (rows == 0) return 0;
    if (dtype == SF_BF16)
        SF_LAUNCH((topk_rank_kernel<sf_bf16>), dim3(rows), dim3(256), 0, stream, (const sf_bf16*)logits, ld, rows, V, S, Spad, off,
                  loss_mask_pad, tgt_ids_pad, t2d_index, Vt, row_map, J, th, row_rank, row_hit);
    else
        SF_LAUNCH((topk_rank_kernel<float>), dim3(rows), dim3(256), 0, stream, (const float*)logits, ld, rows, V, S, Spad, off,
                  loss_mask_pad, tgt_ids_pad, t2d_index, Vt, row_map, J, th, row_rank, row_hit);
    return sf_check_launch("sf_topk_rank");
}
