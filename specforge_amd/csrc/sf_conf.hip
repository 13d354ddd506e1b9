// The draft's confidence per row -- its top-1 softmax probability -- and the per-row calibration / gating fold built from it.
//
// conf = max_j softmax(z)_j = 1 / sum_j exp(z_j - max z): what a dynamic draft tree ranks its nodes by and what a dynamic draft length
// thresholds.  sf_ce_fused forms the row's (max, sum-exp) pair but exports neither, and training overwrites the logits right after, so
// row_conf_kernel streams the row once more in front of the CE.  conf_fold_kernel then turns (conf, row_correct) into per-row 0/1 and
// conf values whose column sums (sf_reduce_sum) are the reliability bins of the step and the drafted / accepted counts of chains gated
// at up to 8 thresholds.
//
// row_conf: HBM-bound, one workgroup per row, every logit read once (2 * V bytes per bf16 row), nothing written to the logits; rows
// without a loss mask read nothing.  conf_fold: HBM-trivial, one thread per row.  Fixed reduction order, plain loads and stores, no
// atomics: bitwise repeatable.
#include "sf_api_internal.h"
#include "sf_util.h"

namespace {

constexpr int CONF_MAX_TAU = 8;
constexpr int CONF_MAX_BINS = 32;
struct ConfThresholds { float tau[CONF_MAX_TAU]; };

// (m, d) <- the (max, sum-exp) pair of the union of two partial rows.  An empty partial is (SF_NEG_BIG, 0): its term is 0 * exp(-huge).
// The difference of the two maxima is formed first and scaled inside sf_exp_fast: exp(m * c - mn * c) loses the result at |m| ~ 3000.
SF_DEVICE void conf_merge(float& m, float& d, float m2, float d2) {
    const float mn = fmaxf(m, m2);
    d = d * sf_exp_fast(m - mn) + d2 * sf_exp_fast(m2 - mn);
    m = mn;
}

// Row r (token row rt = row_map ? row_map[r] : r, (b, s) = (rt / S, rt % S)) reads its loss mask at padded index b*Spad + s + off: the
// addressing of topk_rank_kernel.  The output is indexed by TOKEN row: conf_tok[rt].
template <typename T>
SF_GLOBAL void SF_LAUNCH_BOUNDS(256, 2)
row_conf_kernel(const T* logits, long ld, int V, int S, int Spad, int off, const int* loss_mask_pad, const long long* row_map, long ntok,
                float* conf_tok) {
    SF_SHARED float red[16];
    const int r = (int)blockIdx.x;
    const long long rt = row_map ? row_map[r] : (long long)r;
    if (rt < 0 || rt >= (long long)ntok) return;        // (a wrong host count: nothing read, nothing written; workgroup-uniform)
    const long b = (long)(rt / S), s = (long)rt - b * S;
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    if (loss_mask_pad[b * Spad + s + off] == 0) {       // not scored: the sentinel, no logit read (workgroup-uniform exit, before any barrier)
        if (tid == 0) conf_tok[rt] = -1.f;
        return;
    }
    const T* x = logits + (long)r * ld;
    const int V8 = V >> 3;
    float m = SF_NEG_BIG, d = 0.f;
    auto chunk = [&](const SfRaw8<T>& raw) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = raw.at(i);
        float cm = fmaxf(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])), fmaxf(fmaxf(v[4], v[5]), fmaxf(v[6], v[7])));
        const float mn = fmaxf(m, cm);
        float e[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) e[i] = sf_exp_fast(v[i] - mn);
        // the running sum rescaled when the maximum moves (factor 1 when it does not), plus the chunk's terms added pairwise
        d = d * sf_exp_fast(m - mn) + (((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7])));
        m = mn;
    };
    // four 16-byte chunks in flight per lane, as the fused CE streams its rows (for fp32 a chunk is two 16-byte loads)
    constexpr int PU = 4;
    int c = tid;
    for (; c + (PU - 1) * nt < V8; c += PU * nt) {
        SfRaw8<T> raw[PU];
#pragma unroll
        for (int u = 0; u < PU; ++u) raw[u].ld(x + (long)(c + u * nt) * 8);
#pragma unroll
        for (int u = 0; u < PU; ++u) chunk(raw[u]);
    }
    for (; c < V8; c += nt) {
        SfRaw8<T> raw;
        raw.ld(x + (long)c * 8);
        chunk(raw);
    }
    for (int j = V8 * 8 + tid; j < V; j += nt) conf_merge(m, d, SfElem<T>::ld(x + j), 1.f);     // tail (V % 8)
    // wave butterfly (both lanes of a pair form the same sum: a + b commutes), then the waves in ascending order
    for (int k = 32; k >= 1; k >>= 1) {
        const float m2 = sf_shfl_xor(m, k), d2 = sf_shfl_xor(d, k);
        conf_merge(m, d, m2, d2);
    }
    const int w = tid >> 6, nw = nt >> 6;
    if (sf_lane() == 0) { red[w] = m; red[8 + w] = d; }
    sf_syncthreads();
    if (tid == 0) {
        m = red[0]; d = red[8];
        for (int i = 1; i < nw; ++i) conf_merge(m, d, red[i], red[8 + i]);
        conf_tok[rt] = 1.f / d;     // the maximum's own term is exp(0) = 1, so d >= 1
    }
}

// One thread per row; every output is channel-major [channels, rows], so consecutive lanes store consecutive words.
SF_GLOBAL void SF_LAUNCH_BOUNDS(256, 2)
conf_fold_kernel(int rows, int S, int Spad, int off, long ntok, const int* loss_mask_pad, const long long* row_map, const float* conf_tok,
                 const float* row_correct, int NB, int J, ConfThresholds th, const int* gate_depth, const int* gate_len, float* row_bins,
                 float* row_gate, float* row_draft) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const long long rt = row_map ? row_map[r] : (long long)r;
    const bool inside = rt >= 0 && rt < (long long)ntok;       // (a wrong host count: zeros out)
    bool lm = false, hit = false, open = false;
    float c = -1.f;
    if (inside) {
        const long b = (long)(rt / S), s = (long)rt - b * S;
        lm = loss_mask_pad[b * Spad + s + off] != 0;
        c = conf_tok[rt];
        hit = row_correct[r] != 0.f;
        open = J > 0 && lm && gate_depth[rt] == off;        // the row had a loss mask at every shallower depth
    }
    const bool scored = lm && c >= 0.f;
    if (NB > 0) {
        int bin = (int)(c * (float)NB);     // one fp32 multiply, then truncation
        bin = bin < NB - 1 ? bin : NB - 1;
        for (int q = 0; q < NB; ++q) {
            const bool in = scored && bin == q;
            row_bins[(long)q * rows + r] = in ? 1.f : 0.f;
            row_bins[(long)(NB + q) * rows + r] = in && hit ? 1.f : 0.f;
            row_bins[(long)(2 * NB + q) * rows + r] = in ? c : 0.f;
        }
    }
    for (int j = 0; j < J; ++j) {
        const bool over = c >= th.tau[j];
        row_gate[(long)j * rows + r] = scored && hit && over ? 1.f : 0.f;
        row_draft[(long)j * rows + r] = open && over && gate_len[(long)(1 + j) * ntok + rt] == off ? 1.f : 0.f;
    }
}

}  // namespace

extern "C" int sf_row_conf(const void* logits, int dtype, long ld, int rows, int V, int S, int Spad, int off, const int* loss_mask_pad,
                           const long long* row_map, long ntok, float* conf_tok, void* stream) {
    SF_CHECK_ARG(rows >= 0 && V > 0 && S > 0 && Spad >= S && off >= 0 && off + S <= Spad && ntok >= 0 && ntok % S == 0, "sf_row_conf: bad shape");
    SF_CHECK_ARG(dtype == SF_BF16 || dtype == SF_F32, "sf_row_conf: dtype");
    SF_CHECK_ARG(ld % 8 == 0 && ld >= V && ((size_t)logits & 15) == 0, "sf_row_conf: ld must be a multiple of 8 and >= V, logits 16-byte aligned");
    SF_CHECK_ARG(row_map || (long)rows <= ntok, "sf_row_conf: more dense rows than token rows");
    if (rows == 0) return 0;        // (an empty logits tensor has no address)
    SF_CHECK_ARG(logits && loss_mask_pad && conf_tok, "sf_row_conf: missing input or output");
    if (dtype == SF_BF16)
        SF_LAUNCH((row_conf_kernel<sf_bf16>), dim3(rows), dim3(256), 0, stream, (const sf_bf16*)logits, ld, V, S, Spad, off, loss_mask_pad,
                  row_map, ntok, conf_tok);
    else
        SF_LAUNCH((row_conf_kernel<float>), dim3(rows), dim3(256), 0, stream, (const float*)logits, ld, V, S, Spad, off, loss_mask_pad,
                  row_map, ntok, conf_tok);
    return sf_check_launch("sf_row_conf");
}

extern "C" int sf_conf_fold(int rows, int S, int Spad, int off, long ntok, const int* loss_mask_pad, const long long* row_map,
                            const float* conf_tok, const float* row_correct, int NB, int J, const float* tau, const int* gate_depth,
                            const int* gate_len, float* row_bins, float* row_gate, float* row_draft, void* stream) {
    SF_CHECK_ARG(rows >= 0 && S > 0 && Spad >= S && off >= 0 && off + S <= Spad && ntok >= 0 && ntok % S == 0, "sf_conf_fold: bad shape");
    SF_CHECK_ARG(NB >= 0 && NB <= CONF_MAX_BINS && (NB == 0 || row_bins), "sf_conf_fold: 0 to 32 bins, with row_bins");
    SF_CHECK_ARG(J >= 0 && J <= CONF_MAX_TAU && (J == 0 || (tau && gate_depth && gate_len && row_gate && row_draft)),
                 "sf_conf_fold: 0 to 8 thresholds, with tau, the gate state, row_gate and row_draft");
    SF_CHECK_ARG(NB > 0 || J > 0, "sf_conf_fold: no output");
    SF_CHECK_ARG(row_map || (long)rows <= ntok, "sf_conf_fold: more dense rows than token rows");
    SF_CHECK_ARG(loss_mask_pad && conf_tok && row_correct, "sf_conf_fold: missing input");
    ConfThresholds th;
    for (int j = 0; j < CONF_MAX_TAU; ++j) th.tau[j] = 2.f;
    for (int j = 0; j < J; ++j) {
        SF_CHECK_ARG(tau[j] >= 0.f && tau[j] <= 1.f, "sf_conf_fold: thresholds lie in [0, 1]");
        th.tau[j] = tau[j];
    }
    if (rows == 0) return 0;
    SF_LAUNCH(conf_fold_kernel, dim3((rows + 255) / 256), dim3(256), 0, stream, rows, S, Spad, off, ntok, loss_mask_pad, row_map, conf_tok,
              row_correct, NB, J, th, gate_depth, gate_len, row_bins, row_gate, row_draft);
    return sf_check_launch("sf_conf_fold");
}
