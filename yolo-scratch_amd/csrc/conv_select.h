// Inputs of the conv kernel selection (conv.hip conv_route / eval_route and the planners of conv_*.hip): the policy
// snapshot of one call and the forward / data-gradient view of a descriptor.
#pragma once
#include "common.h"

namespace ym {

// The conv selection policies (the setters of yolomi_experimental.h) as one call saw them.  An entry point loads it
// once and every decision of that call — plan, workspace size, launch instance — reads this copy, so a setter racing
// the call leaves it entirely under the old or entirely under the new value.  The Policy atomics themselves are
// private to conv.hip: a planner cannot read one.
struct ConvPolicy {
    int select_batch;                                   // ym_conv_set_select_batch (0: the real batch)
    int halo, pipe, direct, hpipe;                      // ym_conv_set_halo / _pipe / _direct / _hpipe (-1: default rule)
    int fold;                                           // ym_conv_set_fold
    int eval_cfg, eval_narrow, eval_split, eval_split_nk, eval_gemm_tiles, eval_pipe, eval_route;   // ym_conv_set_eval_*

    static ConvPolicy load();                           // each atomic read exactly once (conv.hip)

    // Conv kernel selection batch (ym_conv_set_select_batch): when > 0 the selection rules of every conv
    // kernel (size thresholds, tile shapes) evaluate as if the batch held this many images, while the
    // launch geometry still follows the real batch — so a small-batch parity test runs exactly the kernel
    // instances a large-batch training step selects.  0 (the default): the real batch.
    int64_t select_n(const ym_conv_desc* d) const { return select_batch > 0 ? int64_t(select_batch) : int64_t(d->n); }
};

// d (always the FORWARD conv's descriptor) as the forward (dir 0) or its data gradient (dir 1) sees it: the tensor
// the kernel gathers from (the input x / the output gradient dz through the y view) and the one it writes
struct ConvSide {
    int kin, nout;                                      // gathered / written channels
    int64_t in_ld, in_bs, out_ld, out_bs;               // pixel / image strides of the gathered and the written view
    int GH, GW, OH, OW;                                 // gathered map, written pixel grid
    int os;                                             // output step: the data gradient of a stride-s conv writes s x s
                                                        // parity classes; the forward 1
};
static inline ConvSide side(const ym_conv_desc* d, int dir) {
    if (!dir) return {d->cin, d->cout, d->x_ld, d->x_bs, d->y_ld, d->y_bs, d->h, d->w, d->oh, d->ow, 1};
    return {d->cout, d->cin, d->y_ld, d->y_bs, d->x_ld, d->x_bs, d->oh, d->ow, d->h, d->w, d->stride};
}

}  // namespace ym
