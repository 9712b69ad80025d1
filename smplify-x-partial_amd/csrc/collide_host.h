// collide_host.h -- what collide.hip offers the host layer (csrc/host/) beyond the sfx_pen_* operators of include/sfx.h.
// Included by collide.hip, which defines these, and by the host units, which call them: one declaration per function.
#pragma once
#include "../../include/sfx.h"
#include "sfx_internal.h"

// sfx_pen_eval on the columns whose want_dev flag is set (NULL: all), writing the adjoint GEMM's operand through `prep` and the
// columns that kept partners by arrival order to over_dev (either may be NULL)
int sfx_pen_eval_masked(sfx_pen* h, int32_t B, const float* verts_dev, float sigma, int32_t penalize_outside,
                        float* loss_dev, float* dverts_dev, const int* want_dev, const PenAdjPrep* prep, int* over_dev, void* stream);
int sfx_pen_capacity(const sfx_pen* h);          // meshes per call the handle's buffers hold
void sfx_pen_note_batch(sfx_pen* h, int B);      // meshes of the evaluation a replayed graph performs
void sfx_pen_reuse(sfx_pen* h);                  // a handle taken from a model's idle slot: per-process settings of the lab build re-read
int sfx_pen_stats_from(const int* stats_dev, int n, int32_t* stats_host);
int sfx_pen_stats_stride(void);
const int* sfx_pen_stats_dev(const sfx_pen* h);
