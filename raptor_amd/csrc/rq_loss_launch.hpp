// rq_loss_launch.hpp - what one loss-and-gradient launch of the learner is (LossLaunch; launch_policy_loss_grad, rq_grad_bank.hpp,
// reads it and the C layer, rq_capi_grad.cpp, fills it), and where the per-wave regions of its workspace lie (loss_partial_layout:
// the one statement of that layout - the launcher carves by it, the C layer reserves by it); and its sibling without a backward, the
// error table's launch (ErrorTableLaunch; launch_policy_error_table), and the gain table's (GainTableLaunch;
// launch_policy_gain_table; tests/gain_launch_driver.cpp holds its defaults).  Host code without a HIP dependency: a
// plain host compiler takes this file alone (tests/loss_launch_driver.cpp does, and holds the layout against tests/test_capi_cpu.py's
// own figures).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/raptor_quad.h"

namespace rq {

// The workspace `partial` of a launch over n envs, in floats from its base (256-byte aligned): every wave of 64 envs leaves its
// partial gradient and its squared error, and what the reduction normalises by - its count of live entries, or, weighted, its sum of
// the counting weights in float64.  A region the form does not have is empty, at `floats`.
struct LossPartialLayout {
    uint32_t waves;
    size_t partial;     // [waves][2084] floats
    size_t wsum;        // weighted: [waves] float64; 2084 waves floats before it, an even number: 8-byte aligned
    size_t sse;         // [waves] floats
    size_t live;        // unweighted: [waves] uint32
    size_t floats;      // all of it
};

constexpr LossPartialLayout loss_partial_layout(uint32_t n, bool weighted) {
    const uint32_t waves = (n + 63) / 64;
    const size_t w = waves, grads = w * RQ_POLICY_NUM_WEIGHTS;
    return weighted ? LossPartialLayout{waves, 0, grads, grads + 2 * w, grads + 3 * w, grads + 3 * w}
                    : LossPartialLayout{waves, 0, grads + 2 * w, grads, grads + w, grads + 2 * w};
}

// One launch: the forward that saves the state, the backward seeded by the masked (weighted) squared error against the target, the
// reduction.  Set the fields by name; what a form does not use keeps its default.
struct LossLaunch {
    uint32_t n = 0, ld = 0, steps = 0;
    // the forward and the transposed operand image (pack_policy, pack_policy_grad).  A bank - block_policy set - has one of each per
    // policy, [n_policies][RQ_PACKED_FLOATS] and [n_policies][RQ_PACKED_GRAD_FLOATS], block_policy [ceil(n / 64)] as the bank's rollout
    // takes it, and the policies' waves as a CSR list: wave_offsets [n_policies + 1] into wave_list [ceil(n / 64)], ascending within
    // a policy.  block_policy null: a single policy.
    const float* packed = nullptr;
    const float* gpacked = nullptr;
    uint32_t n_policies = 0;
    const uint32_t* block_policy = nullptr;
    const uint32_t* wave_offsets = nullptr;
    const uint32_t* wave_list = nullptr;
    // the recording: obs [steps][22][ld], done [steps][ld]; the state before step 0, hidden [16][ld_h], or - start_initial - the learned
    // initial one; saved [steps][16][ld], the state entering every step, written
    const float* obs = nullptr;
    const uint8_t* done = nullptr;
    const float* hidden = nullptr;
    uint32_t ld_h = 0;
    bool start_initial = false;
    float* saved = nullptr;
    const float* target = nullptr;      // y [steps][4][ld_y]; an entry is live where its done code is not 4 and its column < n
    uint32_t ld_y = 0;
    // null: loss = the mean of (a - y)^2 over the live entries.  Else weight [weight_steps][ld_w], weight_steps = 1 (per env) or
    // steps (per env and step), ld_w >= n: an entry counts where it is live and its weight > 0, loss = sum w (a - y)^2 / W4, W4 = the
    // sum of w over the counting entries in float64.  Weights of 1.0f give the unweighted bits.
    const float* weight = nullptr;
    uint32_t ld_w = 0, weight_steps = 0;
    float* partial = nullptr;           // loss_partial_layout(n, weight != nullptr).floats
    // grad [2084] and loss [1]; a bank: grad [n_policies][2084] and loss [n_policies], each policy's over its own blocks (a policy
    // without a wave: loss NaN, its gradient row not written).  Nothing counts: loss 0 and a zero gradient.
    float* grad = nullptr;
    float* loss = nullptr;
    unsigned long long* live = nullptr; // a single policy, unweighted: [1] = the live entries
};

// One error-table launch (launch_policy_error_table, rq_grad_bank.hpp): the forward alone, storing nothing of the pass, and the squared
// imitation error per env and bucket of episode age.  `pass` is read as a loss launch's forward reads it - n, ld, steps, packed (a
// bank: block_policy and n_policies too), obs, done, hidden, ld_h, start_initial, target, ld_y; `saved`, the transposed images, the
// weight, the workspace and the loss outputs are not touched.
constexpr uint32_t kErrorTableMaxBuckets = 32;      // the probe's (rq_probe.hpp kProbeMaxBuckets)
struct ErrorTableLaunch {
    LossLaunch pass;
    uint32_t n_buckets = 0;                           // 1 .. kErrorTableMaxBuckets
    uint32_t edges[kErrorTableMaxBuckets + 1] = {};   // edges[0 .. n_buckets], strictly ascending: bucket b holds ages [edges[b], edges[b + 1])
    // sse [n_buckets][ld_out] and count [n_buckets][ld_out], ld_out >= n: every cell (b, i < n) is written, columns >= n are left
    float* sse = nullptr;
    uint32_t* count = nullptr;
    uint32_t ld_out = 0;
};

// One gain-table launch (launch_policy_gain_table, rq_grad_bank.hpp): the backward's recompute walked forwards with four local seeds,
// storing nothing of the pass, and A = da/dp0 [4][16] summed per env and bucket of episode age.  `pass` is read as the seeded
// backward reads it - n, ld, steps, packed and gpacked (a bank: block_policy and n_policies too), obs, done - plus the forward's
// hidden, ld_h, start_initial; there is no target, and `saved`, the weight, the workspace and the loss outputs are not touched.
struct GainTableLaunch {
    LossLaunch pass;
    uint32_t n_buckets = 0;                           // 1 .. kErrorTableMaxBuckets
    uint32_t edges[kErrorTableMaxBuckets + 1] = {};   // as ErrorTableLaunch's
    // sum [n_buckets][4][16][ld_out], cell (b, i, k, e) = the sum of A_t[i][k] over env e's live steps in bucket b, and count
    // [n_buckets][ld_out], ld_out >= n: every cell with e < n is written, columns >= n are left
    float* sum = nullptr;
    uint32_t* count = nullptr;
    uint32_t ld_out = 0;
};

}  // namespace rq
