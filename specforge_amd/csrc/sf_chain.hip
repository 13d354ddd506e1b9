// Joint accepted length of the draft chains over the TTT steps: the per-row carrier between the steps.
//
// Row s of the [B, S] grid is one draft chain through every TTT step: at step k it consumes its own hidden state of step k-1 and is
// scored against the teacher's token at s + k.  "The chain after position s is accepted to depth d" is "row s hit at steps 0 .. d-1"
// (top-1: the fused CE's row_correct; a full top-k tree: row_hit of sf_topk_rank).  One call per step folds that step's per-row hits
// into two integers per token row: the number of leading steps with a loss mask (chain_depth) and, per channel, the number of leading
// hits (chain_len).  A step without a loss mask censors the chain (it is no miss); a missed step ends it; neither revives.
//
// HBM-trivial: (3 + J) words read and (2 + J) written per row, against 2 * V bytes of logits for the same row and step.  One thread per
// row, channel-major outputs (consecutive lanes store consecutive words), plain loads and stores: bitwise repeatable.
#include "sf_api_internal.h"
#include "sf_util.h"

namespace {

constexpr int CHAIN_MAX = 8;

// Row r (token row rt = row_map ? row_map[r] : r, (b, s) = (rt / S, rt % S)) reads its loss mask at padded index b*Spad + s + off: the
// addressing of topk_rank_kernel.  row_map entries are distinct, so no two threads share a token row's state.
SF_GLOBAL void SF_LAUNCH_BOUNDS(256, 2)
chain_step_kernel(int rows, int S, int Spad, int off, long ntok, const int* loss_mask_pad, const long long* row_map,
                  const float* row_correct, const float* row_hit, int J, int* chain_depth, int* chain_len, float* row_out) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const long long rt = row_map ? row_map[r] : (long long)r;
    bool eligible = false;
    const bool inside = rt >= 0 && rt < (long long)ntok;       // (a wrong host count: zeros out, no state touched)
    if (inside) {
        const long b = (long)(rt / S), s = (long)rt - b * S;
        eligible = loss_mask_pad[b * Spad + s + off] != 0 && chain_depth[rt] == off;
        if (eligible) chain_depth[rt] = off + 1;
    }
    row_out[r] = eligible ? 1.f : 0.f;
    for (int h = 0; h <= J; ++h) {
        bool alive = false;
        if (eligible) {
            const float hit = h == 0 ? row_correct[r] : row_hit[(long)(h - 1) * rows + r];
            int* len = chain_len + (long)h * ntok + rt;
            alive = *len == off && hit != 0.f;
            if (alive) *len = off + 1;
        }
        row_out[(long)(1 + h) * rows + r] = alive ? 1.f : 0.f;
    }
}

}  // namespace

extern "C" int sf_chain_step(int rows, int S, int Spad, int off, long ntok, const int* loss_mask_pad, const long long* row_map,
                             const float* row_correct, const float* row_hit, int J, int* chain_depth, int* chain_len, float* row_out,
                             void* stream) {
    SF_CHECK_ARG(rows >= 0 && S > 0 && Spad >= S && off >= 0 && off + S <= Spad && ntok >= 0 && ntok % S == 0, "sf_chain_step: bad shape");
    SF_CHECK_ARG(J >= 0 && J <= CHAIN_MAX && (J == 0 || row_hit), "sf_chain_step: 0 to 8 top-k channels, with row_hit");
    SF_CHECK_ARG(row_map || (long)rows <= ntok, "sf_chain_step: more dense rows than token rows");
    SF_CHECK_ARG(loss_mask_pad && row_correct && chain_depth && chain_len && row_out, "sf_chain_step: missing input or output");
    if (rows == 0) return 0;
    SF_LAUNCH(chain_step_kernel, dim3((rows + 255) / 256), dim3(256), 0, stream, rows, S, Spad, off, ntok, loss_mask_pad, row_map,
              row_correct, row_hit, J, chain_depth, chain_len, row_out);
    return sf_check_launch("sf_chain_step");
}
