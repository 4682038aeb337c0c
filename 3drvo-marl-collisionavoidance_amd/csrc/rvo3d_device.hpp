// rvo3d_device.hpp -- gfx950 device code of the batched 3D-RVO drone step.
//
// One thread = one drone; a workgroup holds EPB whole environments so the
// whole step (RVO reward sweep -> integrate -> observation sweep -> optional
// auto-reset + re-observe -> outputs) is ONE launch with workgroup barriers
// between the phases.  Neighbour position / velocity / radius / priority are
// staged in LDS (64 B per drone).
//
// Cost structure (fp64 VALU is the scarce resource):
//   * stage G (packed fp32, full lane utilisation): a CONSERVATIVE candidate
//     filter over all neighbours - in range (|dp|^2 <= 100 + band), approaching
//     (v.rel > -eps) or nearly touching - builds a 64-bit candidate mask per
//     lane.  The bands bound the fp32 error (host-computed from the map size),
//     so a pair the reference would act on is never dropped;
//   * stage X (fp64, candidates only) repeats every test exactly: squared norms
//     against T(tau) = max{x : sqrt(x) <= tau} (equivalent to the reference's
//     `norm(..) <= tau` for a correctly rounded sqrt), collision, v.rel, then a
//     conservative cone pre-filter (beta >= alpha + 1e-4 rad, no asin/acos/div)
//     and only for the rest asin / acos / the TTC quadratic;
//   * outputs are quantised without fp64 divisions where that is provably exact
//     after the float32 cast, and observations are written once, coalesced.
//
// Decision arithmetic is fp64 and follows the reference's evaluation order
// (compile with -ffp-contract=off; the explicit __builtin_fma calls model the
// OpenBLAS ddot the reference goes through, see DESIGN.md "arithmetic model").
// Reference citations are relative to the reference root.
//
// Files: rvo3d_params.hpp (parameter blocks), rvo3d_host_setup.hpp (what the host derives for a handle: bands,
// launch geometry, tables, the staged world; host only), rvo3d_math.hpp (arithmetic model, per-drone
// pieces), rvo3d_lds.hpp (LDS views), rvo3d_pairs.hpp (pair pipeline), rvo3d_step.hpp (the step
// kernel), rvo3d_aux_kernels.hpp (resets, tables, classical RVO selection), rvo3d_rvo_rules.hpp (that selection's
// plain-C++ part: the acceler check, the choice among the candidates), rvo3d_rollout_kernels.hpp (the
// trainer's per-step glue: policy heads + sampling, episode bookkeeping), rvo3d_route_kernels.hpp (routes re-drawn on
// the device: per-env replacement, the Philox start / goal sampler), rvo3d_eval_kernels.hpp (the evaluator's:
// action glue, episode records, per-env re-observation), rvo3d_safety_kernels.hpp (safety metrics of the current state:
// separation, building and wall clearance, near pairs; their fold into the episode records), rvo3d_building_kernels.hpp
// (nearest-building rows for the observation: the reference's gate, the k smallest gaps, the widened row),
// rvo3d_motion_kernels.hpp (moving buildings: the per-env records patrol, the per-cell lists are rebuilt in place),
// rvo3d_rvo_city_kernels.hpp (the classical RVO selection with every candidate swept against the buildings),
// rvo3d_orca_rules.hpp / rvo3d_orca_kernels.hpp (the ORCA velocity: one plane per neighbour and building, the four linear
// programs; the converter from a velocity to the step's action), rvo3d_shield_rules.hpp / rvo3d_shield_kernels.hpp (the
// action shield: ORCA's planes and program on the velocity an action would fly), rvo3d_mfma_tiles.hpp (what the three
// matrix-core policy kernels share: operand types, fragment maps, bf16 pack / split, the split product), rvo3d_policy_mlp.hpp (config 3's MLP(256, 256)
// policy step on the matrix cores), rvo3d_policy_mlp_x3.hpp (the same step with split-bf16 products: float32-class), rvo3d_policy_rnn_tiles.hpp (the
// biGRU actor-critic's step for rows with velocity-obstacle rows, in 32-row tiles on the matrix cores).
#pragma once

#include "rvo3d_params.hpp"
#include "rvo3d_math.hpp"
#include "rvo3d_lds.hpp"
#include "rvo3d_pairs.hpp"
#include "rvo3d_step.hpp"
#include "rvo3d_aux_kernels.hpp"
#include "rvo3d_rollout_kernels.hpp"
#include "rvo3d_route_kernels.hpp"
#include "rvo3d_eval_kernels.hpp"
#include "rvo3d_safety_kernels.hpp"
#include "rvo3d_building_kernels.hpp"
#include "rvo3d_motion_kernels.hpp"
#include "rvo3d_rvo_city_kernels.hpp"
#include "rvo3d_orca_kernels.hpp"
#include "rvo3d_shield_kernels.hpp"
#include "rvo3d_mfma_tiles.hpp"
#include "rvo3d_policy_mlp.hpp"
#include "rvo3d_policy_mlp_x3.hpp"
#include "rvo3d_policy_rnn_tiles.hpp"
