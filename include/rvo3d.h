/*
 * rvo3d.h -- C-ABI of the MI355X-native batched 3D-RVO drone environment
 * (librvo3d_hip.so; HIP kernels for gfx950 behind plain-C entry points).
 *
 * The reference (ZSHCRWY25/3DRVO-MARL-CollisionAvoidance) is pure Python and
 * has no FFI of its own; the boundary this library drops in under is the
 * Python surface of `uaisa_env.drone_envs.mdin.mdin`.  Each entry point names
 * the reference method it replaces (paths relative to the reference root).
 * The Python binding a maintainer adds is shown in INTEGRATION.md.
 *
 * Conventions
 *   - E environments x N drones; drone (e, d) has flat index e*N + d.
 *   - Unless marked HOST, every pointer is a DEVICE pointer owned by the
 *     caller (e.g. torch tensors) and only borrowed for the call.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  All
 *     work is enqueued on it; nothing synchronises unless stated.
 *   - Every function returns RVO3D_OK or a negative error; the message for
 *     the calling thread's last error is rvo3d_last_error().  Nothing throws.
 *   - A handle is bound to one device, is not re-entrant, and owns its state
 *     buffers; step/observe allocate nothing.
 */
#ifndef RVO3D_H
#define RVO3D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RVO3D_VERSION 1

enum {
  RVO3D_OK = 0,
  RVO3D_ERR_INVALID = -1,  /* bad argument / unsupported configuration */
  RVO3D_ERR_HIP = -2,      /* a HIP runtime call failed                */
  RVO3D_ERR_STATE = -3     /* call order (e.g. step before load_world) */
};

enum { RVO3D_F32 = 0, RVO3D_F64 = 1, RVO3D_BF16 = 2 };

/* bits of the device error word (rvo3d_error_flags) */
enum {
  RVO3D_FLAG_NONFINITE_OBS = 1, /* an observation held NaN/Inf: the reference
                                   raises ValueError here (ir_gym.py:232-239) */
  RVO3D_FLAG_DOMAIN_ERROR = 2,  /* env_train = 0 only: a pair with r - 0.2 + mr < dis < r + mr
                                   was approaching; the reference's get_alpha raises
                                   ValueError("math domain error") there (vel_obs3D.py:13,
                                   rvo_inter.py:144-165) and aborts the step; here the pair
                                   counts as "no velocity obstacle" and the step completes */
  RVO3D_FLAG_BAD_ROUTE = 4      /* rvo3d_set_routes met an n_points entry outside 2..max_points:
                                   that env kept the routes and the state it had */
};

typedef struct rvo3d_env rvo3d_env;

typedef struct rvo3d_config {
  int32_t num_envs;       /* E >= 1                                            */
  int32_t num_drones;     /* N, 1..512   (data_1.json "drone_num")             */
  int32_t max_points;     /* P >= 2: longest route, in waypoints               */
  int32_t num_buildings;  /* nb >= 0, shared by all envs ("building_list")     */
  int32_t neighbors_num;  /* nm: VO rows kept per observation (mdin.py:7, 10)  */
  int32_t env_train;      /* rvo_inter.py:14 (1 = reference default)           */
  int32_t device;         /* HIP device ordinal                                */
  int32_t action_decimals;/* >= 0: actions are re-quantised on device to that
                             many decimals in fp64 (rint(a*10^d)/10^d), so a
                             float32 buffer of 2-decimal values is widened to
                             exactly the fp64 the reference steps with
                             (multi_ppo.py:205); -1: widen as is               */
  double map_size[3];     /* data_1.json "map_size"                            */
} rvo3d_config;

/* Device views (read-only, see rvo3d_state_ptrs) of the handle's struct-of-arrays state,
 * each [E*N]. Valid until rvo3d_destroy. (reach-through used by the trainer: drone_list[i].vel,
 * multi_ppo.py:202; indicators_*, ir_gym.py:414-420) */
typedef struct rvo3d_state_view {
  double *px, *py, *pz;       /* drone.state                                   */
  double *vx, *vy, *vz;       /* drone.vel                                     */
  double *yaw, *pitch;        /* degrees (drone.py:68-69)                      */
  double *real_len;           /* drone.real_route_len                          */
  double *max_dev;            /* drone.max_deviation                           */
  double *extra_len;          /* drone.extra_len                               */
  int32_t *wp_idx;            /* drone.i                                       */
  uint8_t *arrive, *dest;     /* arrive_flag, destination_arrive_flag          */
} rvo3d_state_view;

/* mdin.__init__ -> ir_gym.__init__ -> env_base.__init__ (mdin.py:7,
 * ir_gym.py:18, env_base.py:15): allocate state for E x N drones. */
int rvo3d_create(const rvo3d_config *cfg, rvo3d_env **out);
int rvo3d_destroy(rvo3d_env *h);

/* env_base.load_data + env_drone.__init__ (env_base.py:26-47,
 * env_drones.py:13-32).  HOST pointers: waypoints [E][N][P][3] (routes shorter
 * than P padded with anything), n_points [E][N] (each 2..P), buildings
 * [nb][4] = x,y,h,r, radius / priority [E][N] or NULL for 0.2 / 5
 * (drone.py:14-15).  Copies to the device, computes route lengths
 * (drone.py:409-429) and puts every drone in its reset state.  Synchronises. */
int rvo3d_load_world(rvo3d_env *h, const double *waypoints, const int32_t *n_points,
                     const double *buildings, const double *radius,
                     const double *priority, void *stream);

/* Per-env building sets.  HOST pointers: buildings [E][nb_max][4] = x,y,h,r; counts [E] (each 0..nb_max; NULL = nb_max
 * for every env).  From the next step on, env e collides with buildings[e][0 .. counts[e]) and with nothing else:
 * exactly the env of a handle whose shared list (rvo3d_load_world) is that list.  The shared list is ignored while
 * sets are attached.  buildings == NULL or nb_max == 0 detaches: back to the shared list.  Needs a loaded world
 * (RVO3D_ERR_STATE otherwise: the lists' reach uses the drones' radii); a later rvo3d_load_world drops the sets.
 * nb_max < 65535 (16-bit indices in the per-cell lists).  Allocates the handle-owned device copies here (freed by the
 * next call / rvo3d_destroy) and synchronises; step and observe still allocate nothing.  Every argument check runs
 * before the first HIP call; a refused call leaves the handle as it was. */
int rvo3d_set_env_buildings(rvo3d_env *h, const double *buildings, const int32_t *counts, int32_t nb_max, void *stream);

/* Moving buildings: advances the records of the attached per-env sets by one time step on the device and rebuilds the
 * per-cell lists where they are - the reference's parked dynamic obstacle (obs_circle: cal_des_vel_omni, full speed
 * towards the goal; move_forward, state += vel * step_time; motion_model.motion_omni), patrolling between two endpoints
 * where the reference's stops at its goal.  m: HOST struct of DEVICE pointers the caller owns, nb_max that of the attached
 * sets; env_mask [E] DEVICE bytes (NULL = every env); buildings_out [E][nb_max][4] DEVICE, nullable.
 * The result is defined by these rules, to the last bit; every value is a float64, every operation rounded on its own (no
 * FMA), a square is x * x, sqrt and / are correctly rounded.  For env e with a non-zero mask byte and its record
 * b = (x, y, h, r), with s = speed[e][b], k = leg[e][b] & 1 and T = ends[e][b][k]:
 *   1. h == -inf (the filler behind counts[e]): nothing else of the record is read, it is not moved, not listed and not
 *      written to buildings_out.
 *   2. step = s * dt.  !(step > 0) - speed 0, a NaN speed, dt 0: the record and leg[e][b] keep their bits (a static
 *      building; its ends are not read).
 *   3. Else dx = T_x - x, dy = T_y - y, d = sqrt(dx*dx + dy*dy).  d <= step: (x, y) = T exactly and leg[e][b] ^= 1; the rest
 *      of the step is not spent.  Else x = x + (dx / d) * step, y = y + (dy / d) * step.  h and r never change.
 *   4. buildings_out[e][b] = the record's four doubles after the move, for every live record (static ones included).
 *   5. Every cell of env e's lists then holds what rvo3d_set_env_buildings computes for the live records where they are
 *      now: the cell widened by 1e-3 m and unbounded at the map's edge, a building listed within min(largest drone
 *      radius + r_b, 5) + 1e-3 of it, in index order, count 0xffff once more than 15 are listed.
 * So a handle whose sets were moved here behaves bit for bit as a handle that was given the same positions through
 * rvo3d_set_env_buildings.  Buildings move before the drones of the same step: call this, then the step, and the step
 * tests the post-move drones against the post-move buildings.  A building may leave the map (the edge cells are
 * unbounded).  Finite ends are the caller's duty.  A later rvo3d_set_env_buildings replaces the records and leaves the
 * caller's leg alone.  Nothing of an env whose mask byte is zero is read or written.
 * One launch, one workgroup per env: no allocation, no synchronisation, no atomics.  RVO3D_ERR_STATE without a loaded
 * world or without attached sets; RVO3D_ERR_INVALID for a null m or a null pointer inside it, and for dt not finite or
 * < 0.  Every argument check runs before the first HIP call and a refused call writes nothing. */
typedef struct rvo3d_building_motion {
  const double *ends;    /* [E][nb_max][2][2]: endpoint 0 and 1, x then y */
  const double *speed;   /* [E][nb_max], metres per unit of dt            */
  uint8_t *leg;          /* [E][nb_max] state: the endpoint being approached */
} rvo3d_building_motion;
int rvo3d_move_env_buildings(rvo3d_env *h, const rvo3d_building_motion *m, double dt, const uint8_t *env_mask,
                             double *buildings_out, void *stream);

/* Per-env drone counts: fleets of different sizes in one handle.  HOST counts [E], each 1..num_drones; NULL detaches
 * (every env has num_drones again).  Env e has the live drones 0 .. counts[e]-1; the rows d >= counts[e] are ghosts.  All
 * layouts stay [E][num_drones].  Env e behaves bit for bit as the env of a handle created with num_drones = counts[e] and
 * loaded with the first counts[e] routes, radii and priorities - state, observations, vo_count, rewards (float32, and
 * float64 when attached), flags, reset_mask and the error word - through every handle-bound entry point: observe, the
 * four step entry points, reset, reset_drones, observe_envs, des_vel, rvo_vel, eval_action, eval_account, set_routes and
 * get_state / set_state; rvo3d_safety_scan and rvo3d_eval_account_safety likewise (their ghost rows are +inf, see there).
 * Ghost rows of every output are defined, and written by every call that writes the live rows (a buffer slot never keeps
 * stale data): the observation row is all zeros; vo_count, reward (+0.0), done, info, finish and reset_mask are 0; the
 * des_vel, rvo_vel and eval_action rows are 0.  Ghost rows of the inputs - actions, drone_mask bytes, the waypoints and
 * n_points of rvo3d_set_routes - are ignored, NaN and out-of-range values included (a bad n_points in a ghost row does
 * not raise RVO3D_FLAG_BAD_ROUTE).  Ghost rows of the state arrays hold the reset state of their unused route and never
 * change (rvo3d_set_state excepted: what it writes there is never read).  The prev_vo_count promise (rvo3d_step_args)
 * keeps its meaning.  rvo3d_eval_account divides `speed` by counts[e]; "all info", "all finish" and "any done" range over
 * the live drones.  The route samplers and the planner draw for all num_drones lanes: the ghosts' routes are unused.
 * Needs a loaded world (RVO3D_ERR_STATE otherwise); a later rvo3d_load_world drops the counts.  num_drones <= 256 (the
 * compile-time rings; RVO3D_ERR_INVALID beyond).  A counted handle of up to 32 drones steps two envs per workgroup on a
 * 32-lane ring, one of up to 64 drones one env on a 64-lane ring: where neighbors_num is so large that this needs more than
 * 64 KiB of LDS the call is refused (RVO3D_ERR_INVALID), although the plain handle may run.  A HIP failure inside the call
 * (RVO3D_ERR_HIP) leaves the counts that were in force in force, but envs may have been reset.  Every env whose count changes ends up in its reset state, as
 * rvo3d_reset leaves it - with extra_len = 0, so that it equals the env of a freshly loaded handle in every state field -
 * and what the step keeps on file is marked stale; envs whose count does not change are not
 * touched.  May allocate and synchronises, like rvo3d_set_env_buildings; step and observe still allocate nothing.  Every
 * argument check runs before the first HIP call; a refused call leaves the handle as it was. */
int rvo3d_set_drone_counts(rvo3d_env *h, const int32_t *counts, void *stream);
/* DEVICE pointer to the counts in force ([E] int32, handle-owned), NULL while none are attached. */
int rvo3d_drone_counts(rvo3d_env *h, const int32_t **device_counts);

/* New routes for the envs whose mask byte is non-zero, from DEVICE memory: waypoints [E][N][P][3] (routes shorter than P
 * padded with anything), n_points [E][N] (each 2..P), env_mask [E] (NULL = every env; the other two are required).  A
 * masked env ends up exactly as an env of a handle freshly loaded (rvo3d_load_world) with these routes: the waypoint rows
 * padded with the destination, n_points, the route lengths (drone.calculate_total_length, drone.py:409-429: the legs in
 * order, a correctly rounded float64 sqrt per leg; a component is squared as x * x, the device's model of the reference's
 * x ** 2, where rvo3d_load_world's host staging calls pow(x, 2): one ulp apart for about 1 leg in 5000), extra_len = 0,
 * the reset state's des_vel and deviation, and every drone of the env in its reset state (drone.reset, drone.py:270-291).  Rows of unmasked envs are neither read nor is
 * anything of those envs written; radius, priority, buildings (the shared list or per-env sets) stay.  An env with an
 * n_points entry outside 2..P is left entirely as it was and raises RVO3D_FLAG_BAD_ROUTE in the device error word (one
 * workgroup per env votes before its first store).  Needs a loaded world (RVO3D_ERR_STATE); a missing pointer is
 * RVO3D_ERR_INVALID; every argument check runs before the first HIP call and a refused call leaves the handle as it was.
 * Enqueues one launch: no synchronisation, no allocation.  The caller observes afterwards (rvo3d_observe). */
int rvo3d_set_routes(rvo3d_env *h, const uint8_t *env_mask, const double *waypoints, const int32_t *n_points,
                     void *stream);
/* The handle's routes as DEVICE copies in the layout rvo3d_load_world takes: waypoints [E][N][P][3] with the padding as
 * stored (the destination behind n_points), n_points [E][N].  Either pointer may be NULL. */
int rvo3d_get_routes(rvo3d_env *h, double *waypoints, int32_t *n_points, void *stream);

/* Start / goal pairs per env from a counter-based generator, written in rvo3d_set_routes' layout; the batched counterpart
 * of uaisa_env/world/random_start_end.py (random pairs with a minimum separation).  No handle: cfg is a HOST struct, the
 * other pointers DEVICE pointers of the current device, work enqueued on `stream`.  For the envs whose mask byte is
 * non-zero (env_mask [E], NULL = every env): waypoints [E][N][P][3] receives the start, the end, and the end again in rows
 * k >= 2; n_points [E][N] receives 2; unplaced [E] (nullable) the number of drones left unplaced, starts plus ends.  Rows
 * of unmasked envs are not written.  The result is defined by these rules, to the last bit:
 *   1. Candidate(kind, e, d, t), kind 0 = start, 1 = end: the Philox4x32-10 block of counter (c0 = low 32 bits of
 *      env_offset + e, c1 = d, c2 = t + kind * 2^31, c3 = draw) under the key (seed low word, seed high word); of its
 *      words x0..x2, u_k = ((double)x_k + 0.5) * 2^-32 and coord_k = rint((lo_k + u_k * (hi_k - lo_k)) * 100.0) / 100.0,
 *      every operation rounded on its own in float64 (no FMA).
 *   2. dist2(a, b) = (dx*dx + dy*dy) + dz*dz in float64, compared with min_sep*min_sep or min_len*min_len.
 *   3. Placement(kind) per env; all drones start unplaced.  In round t = 0 .. max_tries-1 every unplaced drone d takes
 *      c_d = Candidate(kind, e, d, t) and is accepted iff (a) dist2(c_d, p_j) >= min_sep^2 for every j placed in an
 *      earlier round, (b) dist2(c_d, c_j) >= min_sep^2 for every j < d unplaced at the start of round t, accepted in this
 *      round or not, and (c) - ends only - dist2(c_d, start_d) >= min_len^2.  Accepted drones count as placed from the
 *      next round on; a drone still unplaced after the last round keeps its candidate of the last round.
 *   4. Starts are placed first, then ends.
 * env_offset: env e draws as env e + env_offset of a larger batch does (a shard's first env).  Ranges: lo / hi finite with
 * lo < hi, min_sep >= 0, min_len >= 0, max_tries 1..1024, num_envs >= 1, num_drones 1..512, max_points >= 2
 * (RVO3D_ERR_INVALID otherwise; every argument check runs before the first HIP call).  One workgroup per env; no
 * synchronisation, no allocation, no atomics. */
typedef struct rvo3d_route_sampler {
  double lo[3], hi[3];   /* the box                                            */
  double min_sep, min_len;
  int32_t max_tries;
  int32_t reserved;
  uint64_t seed;
  int64_t env_offset;
} rvo3d_route_sampler;
int rvo3d_sample_routes(const rvo3d_route_sampler *cfg, int32_t num_envs, int32_t num_drones, int32_t max_points,
                        uint32_t draw, const uint8_t *env_mask, double *waypoints, int32_t *n_points, int32_t *unplaced,
                        void *stream);

/* The city a route re-draw goes round: a HOST struct whose pointers are DEVICE pointers.  A building is
 * b = (x_b, y_b, h_b, r_b), four doubles.  Env e sees buildings + e * env_stride as [nb_max][4] doubles - env_stride = 0:
 * one list shared by every env, env_stride = nb_max * 4: a set per env - and of those the records 0 .. counts[e]-1
 * (counts == NULL: all nb_max; an entry outside 0 .. nb_max is clamped into that range on the device).  nb_max == 0
 * means no buildings; nb_max < 65535 as for rvo3d_set_env_buildings.  Definitions both calls below share, every value a
 * float64 and every operation rounded on its own (no FMA):
 *   R_b = r_b + clear_xy, top_b = h_b + clear_z, r2(v) = rint(v * 100.0) / 100.0,
 *   max(x, y) = x > y ? x : y, min(x, y) = x < y ? x : y,
 *   inside(p, b) iff ((p_x - x_b)*(p_x - x_b) + (p_y - y_b)*(p_y - y_b)) < R_b*R_b and p_z <= top_b.
 * Checked by both calls before their first HIP call (RVO3D_ERR_INVALID): clear_xy, clear_z finite and >= 0, pad finite
 * and > 0, nb_max in [0, 65535), env_stride 0 or nb_max * 4, buildings non-NULL when nb_max > 0. */
typedef struct rvo3d_city {
  const double *buildings;
  const int32_t *counts;
  int64_t env_stride;      /* doubles per env */
  int32_t nb_max;
  double clear_xy, clear_z; /* the clearance kept from a building's wall and roof */
  double pad;              /* rvo3d_plan_routes: how far outside the clearance cylinder a detour point lies */
} rvo3d_city;

/* rvo3d_sample_routes with one more acceptance rule.  Rules 1, 2, 3 and 4 hold unchanged; rule 3 gains
 *   (d) c_d is accepted only if inside(c_d, b) is false for every building b of its env - starts and ends alike.
 * A candidate refused by (d) still counts as c_j in (b) for the drones behind it, so the rounds stay a parallel vote.
 * With no buildings the outputs equal rvo3d_sample_routes' bit for bit.  pad is checked and not used.  Everything else -
 * arguments, ranges, masking, one workgroup per env, no synchronisation, no allocation, no atomics - as there. */
int rvo3d_sample_routes_city(const rvo3d_route_sampler *cfg, const rvo3d_city *city, int32_t num_envs, int32_t num_drones,
                             int32_t max_points, uint32_t draw, const uint8_t *env_mask, double *waypoints,
                             int32_t *n_points, int32_t *unplaced, void *stream);

/* The detour planner: routes that go round the buildings, in place.  DEVICE pointers: waypoints [E][N][P][3] holds on
 * entry the start in row 0 and the goal in row 1 (the samplers' layout; the other rows are not read) and on return each
 * drone's points with the goal in every row behind them; n_points [E][N] receives the number of points; blocked [E]
 * (nullable) the number of drones of the env whose route FAILED, blocked_mask [E][N] (nullable) one byte per drone, 1 for
 * failed.  env_mask [E] (NULL = every env): nothing of an unmasked env is read or written.  The batched counterpart of
 * the reference's offline Theta* run (uaisa_env/world/theta_star_3D.py); the result is defined by these rules, to the
 * last bit.
 *   Blocks(A, B, b) - is the leg A -> B blocked by b, and at which (t0, tc):
 *     dx = B_x - A_x, dy, dz likewise; a = dx*dx + dy*dy; fx = A_x - x_b, fy = A_y - y_b; c = (fx*fx + fy*fy) - R_b*R_b.
 *     a == 0: blocked iff c < 0 and min(A_z, B_z) <= top_b; t0 = tc = 0.
 *     a != 0: bq = fx*dx + fy*dy; disc = bq*bq - a*c; not blocked unless disc > 0; s = sqrt(disc), correctly rounded;
 *       t0 = (-bq - s) / a, t1 = (-bq + s) / a; not blocked if t1 <= 0 or t0 >= 1; t0 = max(t0, 0), t1 = min(t1, 1);
 *       z0 = A_z + t0*dz, z1 = A_z + t1*dz; blocked iff min(z0, z1) <= top_b; tc = min(max(-bq / a, 0), 1).
 *   FirstBlocker(A, B): the blocking building with the smallest t0, the lowest index among equals (a scan in index order
 *     with a strict <).
 *   Plan, per drone: pts = [start, goal], i = 0; while i < len(pts) - 1, with A = pts[i] and B = pts[i+1]:
 *     no blocker: i += 1.  Otherwise, b being the first blocker: the drone FAILS if len(pts) == P or a == 0; else
 *     l2 = sqrt(a); q = (A_x + tc*dx, A_y + tc*dy); n = q - (x_b, y_b); nl = sqrt(n_x*n_x + n_y*n_y);
 *     if nl < 1e-6: n = (-dy, dx), nl = l2 (the leg runs through the axis: its left normal);
 *     D = (r_b + clear_xy) + pad; W = (r2(x_b + (n_x/nl)*D), r2(y_b + (n_y/nl)*D), r2(A_z + tc*dz));
 *     the drone FAILS if W equals A or B in all three coordinates; else W is inserted behind pts[i] and i stays: the
 *     shortened leg is tested again.
 * A failed drone keeps the points it has: a valid route that still crosses a clearance cylinder.  With no buildings, or
 * with P == 2, no point is ever inserted.  Detours go round a building, never over it.
 * Ranges: the city's (above), num_envs >= 1, num_drones 1..512, max_points >= 2, waypoints and n_points non-NULL
 * (RVO3D_ERR_INVALID otherwise; every argument check runs before the first HIP call).  One workgroup per env, one lane
 * per drone; an env's building records are staged in LDS when there are at most 256 of them and read from global memory
 * otherwise; a drone's points are kept in private memory up to max_points = 16 and in its rows of `waypoints` beyond.
 * One launch: no synchronisation, no allocation, no atomics. */
int rvo3d_plan_routes(const rvo3d_city *city, int32_t num_envs, int32_t num_drones, int32_t max_points,
                      const uint8_t *env_mask, double *waypoints, int32_t *n_points, int32_t *blocked,
                      uint8_t *blocked_mask, void *stream);

/* env_drone.drones_reset (env_drones.py:99) for the envs whose mask byte is
 * non-zero (env_mask NULL = every env). env_mask [E]. */
int rvo3d_reset(rvo3d_env *h, const uint8_t *env_mask, void *stream);
/* mdin.drone_reset_one (mdin.py:43) for every drone whose mask byte is
 * non-zero. drone_mask [E][N]. */
int rvo3d_reset_drones(rvo3d_env *h, const uint8_t *drone_mask, void *stream);

/* ir_gym.env_observation / the observation half of ir_gym.env_reset
 * (ir_gym.py:360-383): observations of every drone with action = 0.
 * obs [E][N][12+9*nm] float32, rows beyond vo_count zero; vo_count [E][N]
 * (0 = the reference's single all-zero VO row). */
int rvo3d_observe(rvo3d_env *h, float *obs, int32_t *vo_count, void *stream);

/* mdin.drone_step (mdin.py:19-30): RVO reward sweep on the pre-move state,
 * kinematic integration, observation / reward / termination sweep on the
 * post-move state.  actions [E][N][3] of action_dtype (RVO3D_F32 / RVO3D_F64).
 * reward [E][N] float32 = rvo_reward + mov_reward (may be inf/nan exactly where
 * the reference's is, ir_gym.py:88); done = collision, info = arrive_flag,
 * finish = destination_arrive_flag (ir_gym.py:248-250), all [E][N] bytes. */
int rvo3d_step(rvo3d_env *h, const void *actions, int32_t action_dtype, float *obs,
               int32_t *vo_count, float *reward, uint8_t *done, uint8_t *info,
               uint8_t *finish, void *stream);

/* rvo3d_step fused with the caller protocol of multi_ppo.py:230-242/266-281:
 * drones with done|finish are reset and every env that reset a drone has all
 * its observations recomputed with action = 0 (ir_gym.env_observation).
 * reset_mask [E][N] (nullable) reports the drones that were reset; reward /
 * done / info / finish are those of the step itself. */
int rvo3d_step_autoreset(rvo3d_env *h, const void *actions, int32_t action_dtype,
                         float *obs, int32_t *vo_count, float *reward, uint8_t *done,
                         uint8_t *info, uint8_t *finish, uint8_t *reset_mask,
                         void *stream);

/* The step driven by raw policy samples: the trainer's glue between `ac.step` and
 * `env.drone_step` (train/policy/multi_ppo.py:196-210) runs on the device, in numpy's
 * own types:  a = np.round(a_inc, 2) (float32);  action = np.round(acceler * a +
 * drone.vel, 2) (float32 product widened, float64 sum).  a_inc [E][N][3] float32;
 * acceler = ir_gym.acceler (0.5).  autoreset != 0 fuses the reset protocol as
 * rvo3d_step_autoreset does (reset_mask nullable). */
int rvo3d_step_policy(rvo3d_env *h, const float *a_inc, float acceler, float *obs,
                      int32_t *vo_count, float *reward, uint8_t *done, uint8_t *info,
                      uint8_t *finish, uint8_t *reset_mask, int32_t autoreset, void *stream);

/* All three step entry points in one, with the arguments in a struct (HOST pointer; the pointers
 * inside it are device pointers as above):
 *   policy == 0: rvo3d_step (autoreset == 0) or rvo3d_step_autoreset (autoreset != 0), actions of
 *                action_dtype;
 *   policy != 0: rvo3d_step_policy, actions = a_inc (float32), acceler, autoreset as there.
 * prev_vo_count (nullable) is a promise about obs: obs and prev_vo_count are a CONSISTENT PAIR - both
 * last written by one observe / step call of this library (prev_vo_count as its vo_count output) and
 * changed by nobody since - so every float of row r past 12 + 9 * prev_vo_count[r] is zero already.  The
 * step then leaves out the stores of those zeros (the fused auto-reset step does; the other paths write
 * in full).  The result is the same as with NULL, which always writes every byte.  prev_vo_count may be
 * the vo_count output itself. */
typedef struct rvo3d_step_args {
  const void *actions;          /* [E][N][3]                                                    */
  int32_t action_dtype;         /* RVO3D_F32 / RVO3D_F64 (policy: ignored, float32)             */
  int32_t policy;               /* != 0: raw policy samples, the trainer glue of rvo3d_step_policy */
  float acceler;                /* policy only: ir_gym.acceler                                  */
  int32_t autoreset;            /* != 0: the fused reset protocol of rvo3d_step_autoreset       */
  float *obs;
  int32_t *vo_count;
  float *reward;
  uint8_t *done, *info, *finish;
  uint8_t *reset_mask;          /* nullable; autoreset only                                     */
  const int32_t *prev_vo_count; /* nullable: see above                                          */
} rvo3d_step_args;
int rvo3d_step_ex(rvo3d_env *h, const rvo3d_step_args *args, void *stream);

/* ---- the trainer's per-step glue around the env step (train/policy/multi_ppo.py:193-281), no handle:
 * plain device pointers, work enqueued on `stream` of the current device ---- */

/* `a, v, logp = ac.step(obs)` (multi_ppo.py:195; policy_rnn_ac.py:57-69, 197-235) from the last hidden
 * layers on, for `rows` observations at once, plus `a = np.round(a, 2)` (:197) and the stores
 * `buf.store(.., a, .., v, logp)` (:217-221): the actor's head (hidden -> 3, tanh), the critic's head
 * (hidden -> 1), a ~ Normal(mu, clamp(std_factor * exp(log_std) + 1e-6, 1e-4, 10)) from a counter-based
 * generator (Philox4x32-10, counter = (row, step), key = seed: reproducible, no generator state), the
 * log-probability of the unrounded sample.  hidden > 0: h_pi / h_v are the hidden activations
 * [rows][ld] of dtype RVO3D_F32 or RVO3D_BF16 (hidden a multiple of 128 resp. 256, at most 1024), the
 * head weights float32 as nn.Linear stores them (w_pi [3][hidden], b_pi [3], w_v [hidden], b_v [1]).
 * hidden == 0: h_pi = mu [rows][ld_pi >= 3] and h_v = v [rows][ld_v >= 1], float32, from the caller's own
 * network (tanh_out ignored).  Outputs: act [rows][3] (rounded: what the buffer stores and
 * rvo3d_step_policy steps from), logp [rows], val [rows]; dbg_mu / dbg_raw [rows][3] nullable. */
typedef struct rvo3d_policy_heads {
  const void *h_pi, *h_v;
  int64_t ld_pi, ld_v;
  int32_t dtype, hidden, tanh_out, reserved;
  const float *w_pi, *b_pi, *w_v, *b_v, *log_std;
} rvo3d_policy_heads;
int rvo3d_policy_sample(const rvo3d_policy_heads *heads, int64_t rows, float std_factor, uint64_t seed,
                        uint64_t step, float *act, float *logp, float *val, float *dbg_mu,
                        float *dbg_raw, void *stream);

/* Config 3's policy step - MLP(256, 256) actor and critic (train/policy/policy_rnn_ac.py:197-257 with the hidden sizes
 * of BASELINE config 3; ac.step, :57-69) - as ONE kernel over the env's observation rows: cast, both hidden layers and
 * the heads on the matrix cores with the activations kept in registers (bf16 operands, float32 accumulation), then what
 * rvo3d_policy_sample does per row (tanh, sample, log-probability, np.round(a, 2), the stores).  Replaces, per rollout
 * step, the observation cast, three GEMMs and rvo3d_policy_sample.
 * rvo3d_policy_mlp_pack turns the nn.Linear tensors (float32, weight [out][in], as the modules store them; widths
 * obs_width -> 256 -> 256 -> 3 for the actor, -> 1 for the critic) into the device blob the kernel reads
 * (rvo3d_policy_mlp_blob_bytes(obs_width) bytes, 16-byte aligned; repack after every optimizer step).
 * obs [rows][obs_ld] float32, obs_width <= 126.  Noise as rvo3d_policy_sample: Philox4x32-10, counter (row, step).
 * vo_count (optional, NULL = none): the env's count output [rows] for these rows.  A row of the env holds state_dim
 * floats, then row_dim floats per velocity-obstacle row, vo_count of them, then zeros: with the counts the
 * kernel neither loads nor multiplies the 16-float column groups that are zero for all 32 rows a wave holds (exactly
 * the same sums: a zero activation adds nothing).  Pass NULL for rows that do not keep that promise. */
typedef struct rvo3d_mlp_weights {
  const float *w1, *b1; /* [256][obs_width], [256] */
  const float *w2, *b2; /* [256][256], [256] */
  const float *w3, *b3; /* [3][256], [3] (actor) or [1][256], [1] (critic) */
} rvo3d_mlp_weights;
int64_t rvo3d_policy_mlp_blob_bytes(int32_t obs_width);
int rvo3d_policy_mlp_pack(const rvo3d_mlp_weights *pi, const rvo3d_mlp_weights *v, int32_t obs_width, void *blob,
                          void *stream);
int rvo3d_policy_mlp_sample(const void *blob, int32_t obs_width, const float *obs, int64_t obs_ld, int64_t rows,
                            const int32_t *vo_count, int32_t state_dim, int32_t row_dim, int32_t tanh_out, const float *log_std, float std_factor, uint64_t seed, uint64_t step,
                            float *act, float *logp, float *val, float *dbg_mu, float *dbg_raw, void *stream);

/* The same policy step at float32-class precision (the reference's policy is float32: train/policy/policy_rnn_ac.py:57-69,
 * :197-235, :238-257).  Every product of the three layers - observation x W1, H1 x W2, H2 x W3 - is split bf16,
 * a_hi b_hi + a_lo b_hi + a_hi b_lo with hi = bf16_rne(x), lo = bf16_rne(x - hi), accumulated in float32 on the matrix
 * cores (the dropped a_lo b_lo is below 2^-16 of each product).  The first layer's bias rides as hi and lo in the
 * weight column obs_width against an exact 1; the second layer's and the heads' biases enter as float32; ReLU acts on
 * the float32 sums and the result is split after it.  Everything else - the per-row tail (tanh, Philox noise with
 * counter (row, step): the same noise as rvo3d_policy_sample and rvo3d_policy_mlp_sample for the same seed and step,
 * log-probability, np.round(a, 2), the stores), vo_count (bit-identical to NULL), the range-checked observation reads,
 * the arguments and their checks - is rvo3d_policy_mlp_sample's.  The blob has its own layout and size
 * (rvo3d_policy_mlp_x3_blob_bytes); repack after every optimizer step. */
int64_t rvo3d_policy_mlp_x3_blob_bytes(int32_t obs_width);
int rvo3d_policy_mlp_x3_pack(const rvo3d_mlp_weights *pi, const rvo3d_mlp_weights *v, int32_t obs_width, void *blob,
                             void *stream);
int rvo3d_policy_mlp_x3_sample(const void *blob, int32_t obs_width, const float *obs, int64_t obs_ld, int64_t rows,
                               const int32_t *vo_count, int32_t state_dim, int32_t row_dim, int32_t tanh_out, const float *log_std, float std_factor, uint64_t seed, uint64_t step,
                               float *act, float *logp, float *val, float *dbg_mu, float *dbg_raw, void *stream);

/* The reader's features (rnn_Reader.obs_rnn + LayerNorm, train/policy/policy_rnn_ac.py:75-127) of rows WITHOUT a
 * velocity-obstacle row, in collapsed form.  The GRU of such a row sees a zero input from h = 0: its hidden state h0 is
 * the same for every row, and LayerNorm(concat(p, h0)) depends on the row only through mean and rstd, so a linear
 * layer W on the features is  W_p f_p + rstd a - (mean rstd) b + c  with a = W_h (h0 g_h), b = W_h g_h, c = W_h b_h + bias
 * (g, b: the LayerNorm's affine).  out [rows][out_ld >= state_dim + 8] receives per row f_p (state_dim floats), rstd as
 * bf16 head, head, tail, mean rstd likewise, 1, 1: the inputs of rvo3d_policy_mlp_sample with obs_width = state_dim + 8
 * and first-layer weights [W_p | a_hi a_lo a_hi | -b_hi -b_lo -b_hi | c_hi c_lo], zero bias (the caller builds them once
 * per optimizer step: rvo3d_amd.policy.policy_rnn_ac.rnn_ac.zero_vo_plan).  sum_h0 / sumsq_h0: the sums of h0 and h0^2,
 * feat_dim = state_dim + hidden.  Rows that do have VO rows get wrong values: the caller recomputes those (below). */
int rvo3d_reader_zero_features(const float *obs, int64_t obs_ld, int64_t rows, int32_t state_dim, int32_t feat_dim,
                               const float *ln_w, const float *ln_b, float sum_h0, float sumsq_h0, float ln_eps,
                               float *out, int64_t out_ld, const int32_t *vo_count, int32_t *list, int32_t *count,
                               void *stream);

/* ... and the rows that DO have velocity-obstacle rows: rvo3d_reader_zero_features, given the env's vo_count, appends
 * their indices to list [rows] (count [1], zero before the first call), and rvo3d_policy_rows computes the policy step
 * of every listed row exactly as the modules do, in float32 (rnn_Reader: the (bi)GRU over the row's vo_count rows,
 * direction sum, concat, LayerNorm - policy_rnn_ac.py:75-168; GaussianActor / Critic stacks state_dim + hidden -> 256
 * -> 256 -> 3 / 1 - :197-257; sample, log-probability, np.round, stores as rvo3d_policy_sample), two workgroups per row
 * (one per network),
 * overwriting what rvo3d_policy_mlp_sample wrote for it; it resets count for the next step (done_blocks [1]: scratch,
 * zero before the first call).  No host synchronisation.  Meant for SHORT lists (a rollout of the benchmark's world has
 * a dozen such rows among 262 144): weights are read as the modules store them, a row is a latency chain of ~35 us. */
typedef struct rvo3d_rnn_policy {
  const float *w_ih_f, *w_hh_f, *b_ih_f, *b_hh_f; /* nn.GRU: [3 hidden][in_dim], [3 hidden][hidden], [3 hidden] x 2 */
  const float *w_ih_r, *w_hh_r, *b_ih_r, *b_hh_r; /* reverse direction, all NULL for a unidirectional GRU */
  const float *ln_w, *ln_b;                       /* [state_dim + hidden] */
  int32_t hidden, in_dim, state_dim, slots;       /* slots = neighbors_num (VO rows per observation) */
  float ln_eps;
  int32_t reserved;
  rvo3d_mlp_weights pi, v;                        /* widths state_dim + hidden -> 256 -> 256 -> 3 / 1 */
} rvo3d_rnn_policy;
int rvo3d_policy_rows(const rvo3d_rnn_policy *net, const float *obs, int64_t obs_ld, const int32_t *vo_count,
                      const int32_t *list, int32_t *count, int32_t *done_blocks, int32_t tanh_out, const float *log_std,
                      float std_factor, uint64_t seed, uint64_t step, float *act, float *logp, float *val, void *stream);

/* The same policy step as rvo3d_policy_rows for the listed rows, built for DENSE lists (worlds where many drones are on a
 * collision course): the rows go in 32-row tiles through the matrix cores (v_mfma_f32_32x32x16_bf16; bf16 operands,
 * float32 accumulation, float32 gate math, LayerNorm and hidden state).  The (bi)GRU runs per row over its vo_count VO
 * rows (forward 0..k-1, reverse k-1..0, as pack_padded_sequence does; directions summed), then concat + LayerNorm, both
 * state_dim + hidden -> 256 -> 256 -> 3 / 1 stacks (ReLU; tanh on mu when tanh_out), and the tail of rvo3d_policy_rows
 * (Philox4x32-10 noise with counter (row, step), log-probability, np.round(a, 2), the stores act / logp / val; dbg_mu
 * [rows][3], nullable, receives mu) - for the listed rows only.  The list (list, count) is sorted on the device into
 * per-count sub-lists in `work` (rvo3d_policy_rnn_tiles_work_bytes(max_rows, slots) bytes, zero before the first call and
 * left zero by every call), so a tile's recurrence is as long as its rows'; the last workgroup out zeroes count and
 * done_blocks [1] (zero before the first call) as rvo3d_policy_rows does.  No host synchronisation; the launch grid does
 * not depend on the count.  `step` is taken by value: this call ignores rvo3d_rollout_set_step_counter's counter.
 * max_rows: the rows of obs / vo_count / act / logp / val / dbg_mu (list entries outside 0..max_rows-1 are skipped).
 * Shapes: hidden 64 or 256, in_dim 9, state_dim 1..16, slots 1..12, GRU or biGRU (bidir), heads (256, 256).
 * rvo3d_policy_rnn_tiles_pack lays out the weights of `net` (float32 as the modules store them, slots ignored) in a
 * device blob of rvo3d_policy_rnn_tiles_blob_bytes(hidden, in_dim, state_dim, bidir) bytes (16-byte aligned; -1 for a
 * shape without an instantiation); repack after every optimizer step.  The call checks blob_bytes against the shape it is
 * given, and the kernel the shape the blob records: a blob packed for another shape computes nothing. */
int64_t rvo3d_policy_rnn_tiles_blob_bytes(int32_t hidden, int32_t in_dim, int32_t state_dim, int32_t bidir);
int rvo3d_policy_rnn_tiles_pack(const rvo3d_rnn_policy *net, void *blob, int64_t blob_bytes, void *stream);
int64_t rvo3d_policy_rnn_tiles_work_bytes(int64_t max_rows, int32_t slots);
int rvo3d_policy_rnn_tiles(const void *blob, int64_t blob_bytes, int32_t hidden, int32_t in_dim, int32_t state_dim,
                           int32_t bidir, const float *obs, int64_t obs_ld, const int32_t *vo_count, const int32_t *list,
                           int32_t *count, int32_t *done_blocks, int32_t *work, int64_t max_rows, int32_t slots,
                           int32_t tanh_out, const float *log_std, float std_factor, uint64_t seed, uint64_t step,
                           float *act, float *logp, float *val, float *dbg_mu, void *stream);

/* The float32-class twin of the trio above (train/policy/policy_rnn_ac.py:57-69, :75-168, :197-257, float32) for float32
 * rollouts and evaluations of the biGRU actor-critic.  Precision model: EVERY product - W_ih x, W_hh h, and here also the
 * three layers of both stacks - is a_hi b_hi + a_hi b_lo + a_lo b_hi of bf16 halves (hi = bf16_rne(x), lo = bf16_rne(x -
 * hi)) with float32 accumulation in one fixed order, so a row's result does not depend on its tile mates; the LayerNorm
 * output and the ReLU'd float32 sums of both hidden layers are split after they are formed; b1 / b2 initialise the float32
 * accumulators, the head biases are added in float32; gate math, LayerNorm and the hidden state are float32.  Against a
 * float64 forward of the modules mu (before the tanh) stays within 1e-4 (mean 1e-5) and v within 1e-4 relative, where the
 * bf16 stacks of rvo3d_policy_rnn_tiles are 1e-3 off.  The noise is that of every other sampling entry point for the same
 * (seed, step): Philox4x32-10 with counter (row, step), the same per-row tail.  Arguments, their checks (all before the
 * first HIP call) and error texts, the list / count / done_blocks / work contract and rvo3d_policy_rnn_tiles_work_bytes
 * are the bf16 trio's.  Blob rules: the blob has its own layout (the stacks' weights as hi and lo fragments), its own
 * magic word and its own, larger size, rvo3d_policy_rnn_tiles_x3_blob_bytes (-1 for the shapes the bf16 query refuses);
 * repack after every optimizer step.  Each call checks blob_bytes against ITS size for the shape - a blob of the other
 * precision is refused with -1 before any launch - and each kernel the magic word and shape the blob records: a blob of
 * the other precision or another shape computes nothing. */
int64_t rvo3d_policy_rnn_tiles_x3_blob_bytes(int32_t hidden, int32_t in_dim, int32_t state_dim, int32_t bidir);
int rvo3d_policy_rnn_tiles_x3_pack(const rvo3d_rnn_policy *net, void *blob, int64_t blob_bytes, void *stream);
int rvo3d_policy_rnn_tiles_x3(const void *blob, int64_t blob_bytes, int32_t hidden, int32_t in_dim, int32_t state_dim,
                              int32_t bidir, const float *obs, int64_t obs_ld, const int32_t *vo_count,
                              const int32_t *list, int32_t *count, int32_t *done_blocks, int32_t *work, int64_t max_rows,
                              int32_t slots, int32_t tanh_out, const float *log_std, float std_factor, uint64_t seed,
                              uint64_t step, float *act, float *logp, float *val, float *dbg_mu, void *stream);

/* Replaying a rollout step as a HIP graph.  The three (MLP policy) or five (biGRU policy) launches of a rollout step take
 * every argument by value, the noise counter `step` included: a captured graph would draw the same noise on every
 * replay.  With a device counter registered here (uint64 in device memory, or NULL to unregister; process-wide), every
 * sampling launch (rvo3d_policy_sample / _mlp_sample / _rows) uses step + *counter, and rvo3d_rollout_account advances
 * the counter by one per call - so a caller captures [policy, rvo3d_step_policy, rvo3d_rollout_account] once per buffer
 * slot and replays it every epoch (rvo3d_amd.policy.multi_ppo, graph_rollout=True; measured on MI355X: the same time
 * per step as the stream launches, 0.158 vs 0.157-0.161 ms). */
int rvo3d_rollout_set_step_counter(uint64_t *device_counter);

/* rnn_Reader.obs_rnn (train/policy/policy_rnn_ac.py:75-127) for observations with AT MOST ONE velocity-obstacle row
 * - nearly all of a rollout's -: the (bi)GRU over a one-step sequence from h = 0 (one cell evaluation per direction,
 * no recurrent product), the sum of the two directions, the concatenation with the proprioceptive part and the
 * LayerNorm, in one pass.  obs [rows][obs_ld] float32 (the env's rows: state_dim proprioceptive floats, then the first
 * VO row of in_dim floats); weights float32 as nn.GRU / nn.LayerNorm store them (w_ih [3 hidden][in_dim], b_ih / b_hh
 * [3 hidden], gates r, z, n; the *_r pointers NULL for a unidirectional GRU; ln_w / ln_b [state_dim + hidden]).
 * feat [rows][feat_ld] of feat_dtype RVO3D_F32 / RVO3D_BF16 receives the state_dim + hidden features (columns beyond
 * stay untouched: the caller's zero padding for the next GEMM).  hidden 64 / 128 / 192 / 256, in_dim 9, state_dim <= 32.
 * Rows whose vo_count exceeds 1 need the full recurrence: the caller recomputes those afterwards. */
typedef struct rvo3d_gru_reader {
  const float *w_ih_f, *b_ih_f, *b_hh_f;
  const float *w_ih_r, *b_ih_r, *b_hh_r;
  const float *ln_w, *ln_b;
  int32_t hidden, in_dim, state_dim;
  float ln_eps;
} rvo3d_gru_reader;
int rvo3d_reader_first_step(const rvo3d_gru_reader *reader, const float *obs, int64_t obs_ld, int64_t rows,
                            void *feat, int32_t feat_dtype, int64_t feat_ld, void *stream);

/* The bookkeeping behind `env.drone_step` in the rollout loop (multi_ppo.py:217-281), for E envs x N drones
 * (N <= 512): the reward into its buffer slot (inf / nan as 0 when sanitize), episode return / length
 * counters, which paths end behind this step (cut_slot [E]: any drone of the env finished or timed out,
 * or the epoch ends - finish_path(0) for every drone of the env, :279), which drones the trainer still has
 * to reset (extra_mask [E][N]: timeouts and, at the epoch's end, everybody the fused step did not reset;
 * *any_extra |= 1 if there is one), and per env the sum / number of finished episodes' returns
 * (sums [E][2], doubles, accumulated: the caller zeroes them and adds them up). */
int rvo3d_rollout_account(int32_t num_envs, int32_t num_drones, const float *reward, const uint8_t *done,
                          const uint8_t *finish, int32_t sanitize, int32_t max_ep_len, int32_t epoch_end,
                          float *rew_slot, float *ep_ret, int32_t *ep_len, uint8_t *cut_slot,
                          uint8_t *extra_mask, double *sums, int32_t *any_extra, void *stream);
/* ... with per-env drone counts: drone_counts is a DEVICE pointer [E] (what rvo3d_drone_counts hands out), NULL = the call
 * above.  Env e's rows d >= drone_counts[e] are ghosts and take no part: their rew_slot and extra_mask bytes are 0, their
 * ep_len / ep_ret stay as they are (0), they never time out, never set cut_slot and never enter sums. */
int rvo3d_rollout_account_n(int32_t num_envs, int32_t num_drones, const int32_t *drone_counts, const float *reward,
                            const uint8_t *done, const uint8_t *finish, int32_t sanitize, int32_t max_ep_len,
                            int32_t epoch_end, float *rew_slot, float *ep_ret, int32_t *ep_len, uint8_t *cut_slot,
                            uint8_t *extra_mask, double *sums, int32_t *any_extra, void *stream);

/* multi_PPObuf.finish_path(0) + get (train/policy/multi_ppo.py:68-91) for every column of a [T][E][N] rollout in ONE
 * launch: rew / val / adv / ret [steps][envs][drones] float32, cut [steps][envs] bytes (any non-zero byte: the paths of
 * that env end behind step t - what rvo3d_rollout_account writes; a torch.bool storage serves as it is).  Per column,
 * from t = steps - 1 down, in float64 (np.append promotes the reference's float32 buffers), every operation rounded on
 * its own as lfilter runs discount_cumsum:
 *     delta = (r[t] + gamma * V[t+1]) - V[t];  adv[t] = delta + (gamma * lam) * adv[t+1];  ret[t] = r[t] + gamma * ret[t+1]
 * with V / adv / ret[t+1] taken as 0 behind a path end; results are stored as float32 (round to nearest even).  The
 * path end is a SELECT, not a multiplication by 0: as in the reference, where every path is an array of its own, an
 * inf / nan reward (sanitize off) makes the steps of its own path before it non-finite and no other.  The byte of row
 * steps - 1 is ignored: the end of the buffer ends every path.  gamma, lam finite; bootstrap value 0 only (the
 * reference's trainer passes no other).  adv and ret must not overlap rew, val, cut or each other (checked:
 * RVO3D_ERR_INVALID).  No handle: plain device pointers of the current device, enqueued on `stream`; every argument
 * check runs before the first HIP call. */
int rvo3d_gae(const float *rew, const float *val, const uint8_t *cut, int64_t steps, int64_t envs, int64_t drones,
              double gamma, double lam, float *adv, float *ret, void *stream);

/* ---- the evaluator's per-step glue around the env step (train/policy/post_train.py:38-128), handle-bound: nothing here
 * synchronises or allocates, every argument check runs before the first HIP call ---- */

/* The evaluator's action (post_train.py:63-74) in numpy's own types: r = rint(a * 100f) / 100f (np.round(a, 2) in
 * float32, a true division), action = (double)(acceler_vel * r) + vel (float32 product widened, float64 sum; unlike
 * rvo3d_step_policy NOT rounded again).  a [E][N][3] float32, action64 [E][N][3] float64 (what rvo3d_step then takes as
 * RVO3D_F64); vel is the handle's own state. */
int rvo3d_eval_action(rvo3d_env *h, const float *a, float acceler_vel, double *action64, void *stream);

/* The episode bookkeeping of post_train.policy_test (:78-105) for every env, after the step and before any reset.
 * Per env: speed = (sum over its drones of sqrt(vx^2 + vy^2 + vz^2)) / N from the handle's post-step velocities, in
 * float64 and in a fixed order (bit-reproducible); speed_sum += speed; ep_ret += (double)reward[e][0]; len = ep_len + 1;
 * the episode ended = any(done) || len == max_ep_len || all(finish)  (==: the trainer's timeout is >).  An env that ended
 * with counted[e] < quota stores the record [e][counted[e]] - len, ep_ret, speed_sum / len, step, flags (1 = all info,
 * 2 = all finish, 4 = any done, 8 = timeout) -, counts it and takes one off *remaining (atomic).  An env that ended has
 * its three running values zeroed, any other stores len; ended[e] = 1 / 0 is written for every env (the mask for
 * rvo3d_reset and rvo3d_observe_envs).  An env past its quota goes on, unrecorded.
 * bufs: HOST struct of device pointers; the running values [E] are zero before the first call, the records [E][quota],
 * remaining [1] set to E * quota by the caller.  reward [E][N] float32, done / info / finish [E][N] bytes (the step's
 * outputs); max_ep_len >= 1, quota >= 1, step: the caller's step number. */
typedef struct rvo3d_eval_bufs {
  int32_t *ep_len;     /* [E] running                                       */
  double *ep_ret;      /* [E]                                               */
  double *speed_sum;   /* [E]                                               */
  int32_t *counted;    /* [E] records of this env so far                    */
  int32_t *rec_len;    /* [E][quota] records                                */
  double *rec_ret;
  double *rec_speed;
  int64_t *rec_step;
  uint8_t *rec_flags;
  int32_t *remaining;  /* [1]                                               */
  uint8_t *ended;      /* [E] written in full by every call                 */
} rvo3d_eval_bufs;
int rvo3d_eval_account(rvo3d_env *h, const float *reward, const uint8_t *done, const uint8_t *info,
                       const uint8_t *finish, int32_t max_ep_len, int32_t quota, int64_t step,
                       const rvo3d_eval_bufs *bufs, void *stream);

/* Safety metrics of the handle's CURRENT state: how close the drones are to each other, to the buildings and to the map
 * faces.  In the evaluator that is the state behind a plain rvo3d_step and before any reset; behind an auto-resetting step
 * the state of an env that was reset is its reset state, so the approach that ended the episode is no longer there.
 * DEVICE outputs, any of them NULL (not computed), but not all four: sep, bclear, wall [E][N] float64, near_pairs [E]
 * int32.  The result is defined by these rules, to the last bit; every value is a float64, every operation rounded on its
 * own (no FMA), a square is x * x, sqrt is correctly rounded.  Env e has the live drones 0 .. n_e-1, n_e = num_drones or,
 * on a counted handle (rvo3d_set_drone_counts), counts[e]; p is a drone's position, r its radius.
 *   1. sep[e][i] = min over the live j != i (by index, not by position) of dis_ij - (r_i + r_j), with rel = p_j - p_i and
 *      dis_ij = sqrt((rel_y*rel_y + rel_x*rel_x) + rel_z*rel_z) (the order of rvo_inter.py's `dis`); +inf in an env of
 *      one live drone.  sep <= 0 holds exactly when dis <= r_i + r_j: the reference's pair collision with env_train = 1
 *      (rvo_inter.py:144).
 *   2. bclear[e][i] = min over the buildings b = (x_b, y_b, h_b, r_b) env e collides with now - its per-env set of
 *      counts[e] records when sets are attached (rvo3d_set_env_buildings), else the shared list - that have p_z <= h_b
 *      (check_col_with_budilding, rvo_inter.py:198-209) of d - (r_i + r_b), d = sqrt(ex*ex + ey*ey), ex = p_x - x_b,
 *      ey = p_y - y_b; +inf when no building counts.  bclear <= 0 is the reference's building hit (but for its 5 m gate,
 *      which can only matter where r_i + r_b > 5).
 *   3. wall[e][i] = m + 0.0, m = the minimum over the axes k = 0, 1, 2 of p_k and of map_k - p_k.  wall < 0 holds exactly
 *      when drone_out_map is true (drone.py:213-225).  (The + 0.0 turns the -0.0 of a coordinate that is -0.0 into +0.0:
 *      no output is ever -0.0.)
 *   4. near_pairs[e] = the number of unordered live pairs i < j with dis_ij - (r_i + r_j) <= near_margin, colliding pairs
 *      included.  near_margin is finite and >= 0 (RVO3D_ERR_INVALID otherwise).
 *   5. A minimum starts from +inf and takes x < m ? x : m.  For finite positions no candidate is NaN and none is -0.0, so
 *      the three minima, like the integer count, do not depend on the order of evaluation: the result is the same bits
 *      for every launch geometry.
 *   6. Ghost rows (d >= n_e) of sep, bclear and wall are written as +inf by every call, so that a min over a row needs no
 *      mask - a deliberate exception to the zeros every other output holds in its ghost rows.  Ghost rows of the state
 *      are never read.
 * One lane per drone, the env's positions and radii staged in LDS once, the buildings in tiles; fleets of up to 64
 * drones share a wave (several envs per wave), larger ones take one workgroup per env.  One launch: no allocation, no
 * synchronisation, no atomics.  Needs a loaded world (RVO3D_ERR_STATE); every argument check runs before the first HIP
 * call and a refused call writes nothing. */
int rvo3d_safety_scan(rvo3d_env *h, double near_margin, double *sep, double *bclear, double *wall,
                      int32_t *near_pairs, void *stream);

/* rvo3d_eval_account with the safety metrics folded into the episode records.  What it does to `bufs` is exactly what
 * rvo3d_eval_account does (the same per-env decision, the same kernel body).  In addition, per env, with this step's
 * values s = (min over the env's live drones of sep, of bclear, of wall; near_pairs) from rvo3d_safety_scan's rules on the
 * current state (after the step, before any reset): folded = (min(s.sep, ep_min_sep), min(s.bclear, ep_min_bclear),
 * min(s.wall, ep_min_wall), ep_near + s.near_pairs), minima by rule 5; where rvo3d_eval_account stores a record, the four
 * folded values go to the same slot of rec_*; an env whose episode ended goes on with (+inf, +inf, +inf, 0), any other
 * with the folded values.  sbufs: HOST struct of device pointers; the caller sets the running values to +inf and 0 before
 * the first call.  Two launches: the scan, into per-env scratch the handle owns (allocated by rvo3d_load_world: this call
 * allocates nothing), and the account.  Arguments and checks as rvo3d_eval_account, near_margin as rvo3d_safety_scan. */
typedef struct rvo3d_eval_safety_bufs {
  double *ep_min_sep, *ep_min_bclear, *ep_min_wall;   /* [E] running, +inf before the first call */
  int64_t *ep_near;                                   /* [E] running sum of near_pairs, 0 before */
  double *rec_min_sep, *rec_min_bclear, *rec_min_wall;/* [E][quota] records                      */
  int64_t *rec_near;                                  /* [E][quota]                              */
} rvo3d_eval_safety_bufs;
int rvo3d_eval_account_safety(rvo3d_env *h, const float *reward, const uint8_t *done, const uint8_t *info,
                              const uint8_t *finish, int32_t max_ep_len, int32_t quota, int64_t step,
                              const rvo3d_eval_bufs *bufs, double near_margin,
                              const rvo3d_eval_safety_bufs *sbufs, void *stream);

/* Nearest-building rows of the handle's CURRENT state (positions, velocities, radii): per drone the k buildings with
 * the smallest gap among those that pass the reference's gate, six floats each - what the reference collects for its
 * observation (rvo_inter.preprocess, rvo_inter.py:85-107; ir_gym.observation_reward, ir_gym.py:216-219) and then leaves
 * out of it (:229), with the time to the building's cylinder it defines and never calls (cal_exp_tim_with_building,
 * rvo_inter.py:248-275).  The buildings are those env e collides with now: its per-env set while sets are attached
 * (rvo3d_set_env_buildings; unused records hold h = -inf and fail the height gate), else the shared list.  Behind an
 * auto-resetting step the state of a drone that was reset is its reset state (velocity 0, urg 0): the state its
 * re-observed row describes.
 * args: HOST struct of DEVICE pointers.
 *   Stand-alone mode (obs == NULL): only the columns col0 .. col0 + 6k - 1 of every output row are written, every other
 *   float of the buffer is left alone.  Needs col0 >= 0 and row_ld >= col0 + 6k.
 *   Widen mode (obs != NULL; W = 12 + 9 * neighbors_num): the whole wide row [ 12 proprio | 6k building | 9 * nm VO ] -
 *   columns 0..11 = obs[g][0..11], 12 .. 12 + 6k - 1 the building floats, 12 + 6k .. W + 6k - 1 = obs[g][12 .. W - 1];
 *   columns behind W + 6k are not written.  Needs col0 == 12 and row_ld >= W + 6k; obs must not overlap rows.  The wide
 *   row keeps what the policy kernels rely on, with state_dim = 12 + 6k: state floats, vo_count rows of 9, then zeros.
 * The result is defined by these rules, to the last bit; every value is a float64, every operation rounded on its own (no
 * FMA), a square is x * x, sqrt and / are correctly rounded, r2(v) = rint(v * 100.0) / 100.0 (np.round(v, 2)).  For a
 * live drone with position p, velocity v, radius r and the building b = (x_b, y_b, h_b, r_b), in index order:
 *   1. Gate: ex = p_x - x_b, ey = p_y - y_b, d = sqrt(ex*ex + ey*ey); b passes iff h_b > p_z - below and d <= reach
 *      (the reference: below = 2, reach = 5).
 *   2. gap = d - (r + r_b): the term rvo3d_safety_scan minimises for bclear.
 *   3. t, with R = r + r_b: a = v_x*v_x + v_y*v_y, bq = (2.0*ex)*v_x + (2.0*ey)*v_y, c = (ex*ex + ey*ey) - R*R.
 *      c <= 0: t = 0.  Else disc = bq*bq - (4.0*a)*c; disc <= 0: t = +inf.  Else s = sqrt(disc), t1 = (-bq + s) / (2.0*a),
 *      t2 = (-bq - s) / (2.0*a), a root that is not >= 0 counts as +inf, t = t2' < t1' ? t2' : t1'.
 *      urg = 1.0 / (t + 0.2): the VO rows' input_exp_time (rvo_inter.py:189); 0 for t = +inf, 5 inside the cylinder.
 *      The time is the reference's, in the plane; column 2 tells whether the roof is below the drone.
 *   4. Row, each as float32 of r2(.) + 0.0 (no output is -0.0):
 *        [ r2(x_b - p_x), r2(y_b - p_y), r2(h_b - p_z), r2(r_b), r2(gap), r2(urg) ]
 *   5. Of the passing buildings the k with the smallest gap are kept, among equal gaps the lower index first, and stored
 *      by ascending (gap, index).  b_count = min(k, passing); rows from b_count on are zeros.  The key includes the
 *      index, so the result does not depend on the launch geometry or the tile order.
 *   6. Ghost rows (counted handle, d >= counts[e]): building floats zeros, b_count 0, in widen mode the whole wide row
 *      zeros; the ghost's state is not read.
 * One lane per drone, the buildings through LDS in tiles, the k slots in registers; the geometry of rvo3d_safety_scan.
 * The rows leave through LDS: consecutive lanes write consecutive floats of a row.  One launch: no allocation, no
 * synchronisation, no atomics.  Needs a loaded world (RVO3D_ERR_STATE); every argument check (RVO3D_ERR_INVALID) runs
 * before the first HIP call and a refused call writes nothing. */
typedef struct rvo3d_building_rows_args {
  int32_t k;          /* rows per drone, 1..8                                         */
  double reach;       /* centre-distance gate, finite > 0   (reference: 5.0)          */
  double below;       /* height gate, finite >= 0           (reference: 2.0)          */
  float *rows;        /* row g = e*N+d starts at rows + g*row_ld                      */
  int64_t row_ld;     /* floats per output row                                        */
  int32_t col0;       /* first column of the 6*k building floats in an output row     */
  int32_t *b_count;   /* [E][N], nullable: rows written for the drone, 0..k           */
  const float *obs;   /* nullable: dense observation [E][N][W], W = 12 + 9*nm         */
} rvo3d_building_rows_args;
int rvo3d_building_rows(rvo3d_env *h, const rvo3d_building_rows_args *args, void *stream);

/* rvo3d_building_rows for buildings that move (rvo3d_move_env_buildings): rows of EIGHT floats,
 *   [ dx, dy, dh, r_b, gap, urg_rel, vb_x, vb_y ],
 * the urgency taken at the drone's velocity relative to the building's - cal_exp_tim_with_building takes a relative
 * velocity (rvo_inter.py:248-275) - and the building's velocity behind it.  args as for rvo3d_building_rows with 8k in
 * place of 6k throughout: stand-alone mode writes the columns col0 .. col0 + 8k - 1 and needs row_ld >= col0 + 8k; widen
 * mode writes [ 12 proprio | 8k building | 9 * nm VO ], needs col0 == 12 and row_ld >= W + 8k, leaves the columns behind
 * W + 8k alone, and obs must not overlap the W + 8k floats of any row.  motion: HOST struct of the DEVICE pointers handed
 * to rvo3d_move_env_buildings (nb_max that of the attached sets), all three read-only here, or NULL: every building stands.
 * dt: that call's.
 * The result is defined by these rules, to the last bit; every value is a float64, every operation rounded on its own (no
 * FMA), a square is x * x, sqrt and / are correctly rounded, r2(v) = rint(v * 100.0) / 100.0 + 0.0.
 *   1. Gate, gap, selection (the k smallest (gap, index)), b_count, the ordering, zero rows from b_count on and ghost
 *      rows are rule for rule those of rvo3d_building_rows: for any motion the same buildings are kept in the same
 *      slots, and columns 0..4 of every row of eight are bit for bit columns 0..4 of the row of six.
 *   2. The velocity vb of the record b = (x, y, h, r) of env e where it stands now, as its next move will be, with
 *      s = speed[e][b], T = ends[e][b][leg[e][b] & 1], step = s * dt:
 *        motion == NULL, or !(step > 0) - speed 0, a NaN speed, dt 0: vb = (0, 0); ends is not read.
 *        Else dx = T_x - x, dy = T_y - y, d = sqrt(dx*dx + dy*dy).  d <= step: vb = (dx / dt, dy / dt) - the next move
 *        lands on T exactly.  Else vb = ((dx / d) * s, (dy / d) * s).
 *      The same rule for every env (no env_mask is known here).  A filler (h == -inf) never passes the gate: nothing of
 *      its motion is read.
 *   3. urg_rel = 1.0 / (t + 0.2), t by rule 3 of rvo3d_building_rows at the velocity (v_x - vb_x, v_y - vb_y) in place of
 *      (v_x, v_y); ex, ey and R as there.
 *   4. Row, each as float32 of r2(.): the five columns of rule 1, r2(urg_rel), r2(vb_x), r2(vb_y).  No output is -0.0.
 *   5. motion == NULL: columns 0..5 are rvo3d_building_rows' six floats bit for bit, columns 6 and 7 are +0.0.
 * The launch is rvo3d_building_rows' (geometry, tiles, slots; the stage holds 8k + 1 dwords per lane); only the row
 * writer differs: for each of its at most k kept records it also reads speed, leg and one endpoint.  One launch: no
 * allocation, no synchronisation, no atomics.  The motion's buffers are the ones rvo3d_move_env_buildings writes: call
 * both on the same stream, this one behind the step.  Graph capture with a motion stays the caller's to refuse.
 * Every argument check runs before the first HIP call and a refused call writes nothing: what rvo3d_building_rows refuses
 * (with 8k); RVO3D_ERR_STATE for a motion without attached per-env sets; RVO3D_ERR_INVALID for a null pointer inside
 * motion and for dt not finite or < 0 (checked with and without a motion).  motion == NULL is allowed on any loaded
 * handle, the shared list included. */
int rvo3d_building_rows_moving(rvo3d_env *h, const rvo3d_building_rows_args *args,
                               const rvo3d_building_motion *motion, double dt, void *stream);

/* rvo3d_observe for the envs whose mask byte is non-zero (env_mask [E], required): their rows of obs / vo_count receive
 * bit for bit what rvo3d_observe writes, the other envs' rows are not written at all - an env in mid-episode keeps the
 * observation of its step (ir_gym.observation_reward, with the action), as in the reference, which observes with
 * action = 0 only behind a reset.  Implemented as the full observation into the caller's scratch pair (scratch_obs /
 * scratch_cnt: the shapes of obs / vo_count, distinct from them) and a row select, so the handle's derived state
 * (des_vel on file, stage-G words, max_dev) is what rvo3d_observe leaves. */
int rvo3d_observe_envs(rvo3d_env *h, const uint8_t *env_mask, float *obs, int32_t *vo_count, float *scratch_obs,
                       int32_t *scratch_cnt, void *stream);

/* mdin.drone_step returns its rewards as Python floats (mdin.py:28: rvo_reward + mov_reward in
 * float64).  Attach a device buffer reward64 [E][N] and every following step (all three step
 * entry points) also writes the float64 value next to the float32 one; NULL detaches.  The
 * buffer is borrowed until detached or the handle is destroyed. */
int rvo3d_set_reward_f64(rvo3d_env *h, double *reward64);

/* ir_gym.cal_des_list (ir_gym.py:44): desired velocity, des_vel [E][N][3] f64. */
int rvo3d_des_vel(rvo3d_env *h, double *des_vel, void *stream);

/* reciprocal_vel_obs.cal_vel (uaisa_env/vel_obs/reciprocal_vel_obs.py:19-31) for every drone
 * on the current state: candidate velocities on a 0.5 grid inside clip([v - acceler,
 * v + acceler], -vmax, vmax), |v| >= 0.3, tested against the reciprocal velocity obstacle
 * of every drone within 10 m; the one closest to the desired velocity outside all cones,
 * else the inside one with the least penalty, else 0.  The reference class cannot run as
 * written; this is the algorithm it spells out, on the helper functions it calls
 * (parity unpinned for the driver loop).  vmax: HOST [3]; 0 <= acceler
 * <= 1; out_vel [E][N][3] f64. */
int rvo3d_rvo_vel(rvo3d_env *h, const double *vmax, double acceler, double *out_vel,
                  void *stream);

/* rvo3d_rvo_vel that also keeps clear of the buildings, standing or moving (rvo3d_move_env_buildings): what
 * reciprocal_vel_obs.preprocess collects as obs_list ("to be filled", reciprocal_vel_obs.py:46-52) and then drops.  Every
 * candidate velocity is swept against the cylinder of every building near the drone over a look-ahead horizon, and the
 * selection is made in four tiers.  motion, dt: as for rvo3d_building_rows_moving - motion is a HOST struct of the DEVICE
 * pointers handed to rvo3d_move_env_buildings, read-only here, or NULL: every building stands (allowed on any loaded
 * handle, the shared list included).
 * The result is defined by these rules, to the last bit; every value is a float64, every operation rounded on its own (no
 * FMA), a square is x * x, sqrt and / are correctly rounded, a minimum starts from +inf and takes x < m ? x : m.
 *   0. Candidates.  The candidates, their numbering c = (ix * cnt_y + iy) * cnt_z + iz, their values, the live set
 *      (|c| >= 0.3), the cone set (inside some neighbour's reciprocal cone) and tc_min (the least cal_exp_tim over the
 *      neighbours within 10 m at the current velocity) are exactly rvo3d_rvo_vel's; live_mask, cone_mask and tc_min
 *      report them.  des is the des_vel rvo3d_rvo_vel uses.
 *   1. Buildings.  Env e's buildings are its per-env set while sets are attached, else the shared list, in index order.
 *      The velocity vb of a record is rule 2 of rvo3d_building_rows_moving (the velocity its next move will have), (0, 0)
 *      without a motion.  Gate (reciprocal_vel_obs.preprocess): ex = p_x - x_b, ey = p_y - y_b,
 *      d = sqrt(ex*ex + ey*ey); b passes iff h_b > p_z - below and d <= reach.  A filler (h = -inf) fails, and nothing of
 *      its motion is read.  n_gated is the number that pass.
 *   2. Swept test, for a passing b and a live candidate (cx, cy, cz): R = (r + r_b) + clear_xy, H = h_b + clear_z,
 *      wx = cx - vb_x, wy = cy - vb_y, a = wx*wx + wy*wy, bq = (2.0*ex)*wx + (2.0*ey)*wy, cq = (ex*ex + ey*ey) - R*R.
 *        cq <= 0 (inside the clearance disk now): t_in = 0; t_out = +inf if a == 0, else
 *          (-bq + sqrt(bq*bq - (4.0*a)*cq)) / (2.0*a).
 *        Else disc = bq*bq - (4.0*a)*cq; disc <= 0: b does not block c.  s = sqrt(disc), t_in = (-bq - s) / (2.0*a),
 *          t_out = (-bq + s) / (2.0*a); !(t_in >= 0): b does not block c (moving away).
 *      b blocks c iff t_in <= horizon and zmin <= H, with te = t_out < horizon ? t_out : horizon, z_in = p_z + cz*t_in,
 *      z_e = p_z + cz*te, zmin = z_e < z_in ? z_e : z_in: the exact sweep of the drone's centre against the cylinder over
 *      the horizon.  A candidate that climbs over the roof before it arrives is free; one that sinks onto a roof it hovers
 *      over is blocked.  Bit c of blocked_mask is the OR over the passing buildings; tb(c) is the minimum of t_in over the
 *      buildings that block c.  For finite state whose squares do not overflow no NaN arises: inside the disk the root is
 *      taken of a sum of two non-negative numbers, outside of disc > 0 only, a quotient 0/0 (a == 0 by underflow) fails
 *      t_in >= 0, and a blocking t_in lies in [0, horizon].  OR and minimum do not depend on the order of the buildings,
 *      so the tile order cannot show in the result.
 *   3. Selection, dd(c) rvo3d_rvo_vel's distance to des, "first" the lowest c:
 *        tier 1: live & ~cone & ~blocked not empty - the least dd, first among equals;
 *        tier 2: else live & ~blocked not empty - the least 1 * tc_inv + dd (rvo3d_rvo_vel's inside rule), first among
 *                equals: buildings do not give way, drones do;
 *        tier 3: else live not empty - the largest tb(c), then the least dd, then the first: every candidate hits
 *                something within the horizon, so take the one that hits last;
 *        tier 4: else out_vel = 0.
 *      A live row's tier is 1..4.
 *   4. Ghost rows (counted handle, d >= counts[e]): out_vel 0 and every diagnostic 0 (tier 0); the ghost's state is not read.
 *   5. When no building passes the gate for a drone, tiers 1 and 2 are rvo3d_rvo_vel's two cases and its out_vel row is
 *      rvo3d_rvo_vel's, bit for bit.
 * rvo3d_rvo_vel's geometry: one workgroup per env, one lane per drone; the building records go through LDS in tiles, the
 * velocity of a record computed once by the lane that loads it; the planar roots are taken once per building and
 * (ix, iy); tier 3 is a second trip over the tiles, entered only when some drone of the env needs it.  One launch: no
 * allocation, no synchronisation, no atomics.  Call it on the stream of rvo3d_move_env_buildings.  Graph capture with a
 * motion stays the caller's to refuse.
 * Every argument check runs before the first HIP call and a refused call writes nothing: RVO3D_ERR_STATE without a loaded
 * world, or for a motion without attached per-env sets; RVO3D_ERR_INVALID for a null args / out_vel / pointer inside
 * motion, for acceler outside [0, 1], for each non-finite or out-of-range double, and for dt not finite or < 0 (checked
 * with and without a motion). */
typedef struct rvo3d_rvo_city_args {
  double vmax[3]; double acceler;          /* as rvo3d_rvo_vel: 0 <= acceler <= 1                          */
  double reach, below;                     /* building gate, finite > 0 / finite >= 0 (reference: 10, 1)   */
  double horizon;                          /* finite > 0: look-ahead, in the time unit of the velocities   */
  double clear_xy, clear_z;                /* finite >= 0: extra clearance round the cylinder / over the roof */
  double *out_vel;                         /* DEVICE [E][N][3], required                                   */
  /* DEVICE, each nullable: what the selection was made from (tests, diagnostics) */
  uint64_t *live_mask, *cone_mask, *blocked_mask;   /* [E][N], bit c = candidate c  */
  double *tc_min;  int32_t *n_gated, *tier;         /* [E][N]                        */
} rvo3d_rvo_city_args;
int rvo3d_rvo_vel_city(rvo3d_env *h, const rvo3d_rvo_city_args *args,
                       const rvo3d_building_motion *motion, double dt, void *stream);

/* The ORCA velocity of every drone on the current state: van den Berg, Guy, Lin, Manocha, "Reciprocal n-body collision
 * avoidance" in three dimensions - one half-space of permitted velocities per neighbour and per building, and the
 * velocity nearest the preferred one in their intersection, by the authors' incremental linear programs.  When every
 * drone applies its result the drones do not collide for time_horizon.  Nothing of this is in the reference; the rules
 * are the published algorithm's, restated in tests/orca_ref.py.  motion, dt: as for rvo3d_rvo_vel_city.
 * The result is defined by these rules, to the last bit; every value is a float64, every operation rounded on its own (no
 * FMA), a square is x * x, a . b = (a_x*b_x + a_y*b_y) + a_z*b_z, |a| = sqrt(a . a), a x b the usual cross product, sqrt
 * and / are correctly rounded, a vector is divided by a scalar component by component.
 *   1. Preferred velocity.  pref = pref_speed * des, des the des_vel rvo3d_rvo_vel uses.
 *   2. Neighbours.  The other drones j of the env (on a counted handle: its live ones) with rel = p_j - p_i and
 *      d2 = rel . rel < neighbor_dist * neighbor_dist; the max_neighbors with the least (d2, j) are kept, in that order.
 *      Priorities are not used: every drone takes half.  n_neighbors is the number kept.
 *   3. Buildings.  Env e's buildings as in rule 1 of rvo3d_rvo_vel_city, with its gate (h_b > p_z - below and d <= reach)
 *      and its velocity vb.  The max_buildings with the least (gap, index) are kept, gap = d - (r + r_b), in that order;
 *      n_buildings is the number kept.  A building is an upright cylinder of unlimited height that takes no share:
 *      rel = (x_b - p_x, y_b - p_y, 0), w_rel = (v_x - vb_x, v_y - vb_y, 0), R = (r + r_b) + clear_xy.  Its plane's
 *      normal is planar: it constrains (v_x, v_y) only.  A drone that is above a roof by less than `below` is therefore
 *      treated as beside that cylinder, not over it: it is pushed out sideways.
 *   4. The plane of an agent (rel, w_rel = v_i - v_j, R; share 0.5 for a drone, 1 for a building), tau = time_horizon:
 *        d2 > R*R:  w = w_rel - rel / tau, dp = w . rel.
 *          dp < 0 and dp*dp > (R*R) * (w . w) (the cut-off circle):  n = w / |w|, u = (R / tau - |w|) n.
 *          else (a leg):  a = d2, b = rel . w_rel, cr = rel x w_rel, c = w_rel . w_rel - (cr . cr) / (d2 - R*R),
 *            t = (b + sqrt(max(b*b - a*c, 0))) / a, ww = w_rel - t rel, n = ww / |ww|, u = (R*t - |ww|) n.
 *        d2 <= R*R (overlapping now):  w = w_rel - rel / time_step, n = w / |w|, u = (R / time_step - |w|) n.
 *      point = v_i + share * u; the half-space is n . (v - point) >= 0.  Guards: max(x, 0) is x > 0 ? x : 0 (0 for a NaN);
 *      a zero-length w takes n = (1, 0, 0).  A zero-length ww - w_rel exactly on the cone's axis, two drones exactly
 *      head-on - is where the published quotient is 0 / 0 and every normal of the cone round its axis is equally near;
 *      (1, 0, 0) for both drones would move both the same way and avoid nothing, so the normal towards perp = e x rel
 *      is taken, e = (0, 0, 1), or (1, 0, 0) when rel_x = rel_y = 0:
 *        n = (sqrt(d2 - R*R) / |rel|) (perp / |perp|) - (R / |rel|) (rel / |rel|),
 *      the limit of ww / |ww| from that side.  The other drone, with -rel, takes -n, as reciprocity needs, and a planar
 *      pair stays planar.  The published library multiplies by 1 / tau where this divides by tau.
 *      No NaN arises for finite state whose squares neither overflow nor underflow to the point that
 *      (cr . cr) / (d2 - R*R) overflows.
 *   5. Order.  Building planes first, by ascending (gap, index), then drone planes by ascending (d2, j).
 *   6. The program: the authors' four (on a line, on a plane, in space, and the fallback that minimises the largest
 *      penetration when the planes have no common point), EPS = 1e-5, for the point of the ball |v| <= max_speed nearest
 *      pref; csrc/rvo3d_orca_rules.hpp is the statement, operation for operation.  Beyond the published text: a point
 *      projected onto a plane that coincides with the plane circle's centre stays there; on a line the discriminant
 *      test is !(disc >= 0).  In the fallback the building planes are hard, as the authors' 2-D library treats obstacle
 *      lines: they enter every projected problem unchanged, only drone planes are relaxed.  When the building planes
 *      themselves have no common point in the ball (max_speed too small to get away from a moving building, a drone
 *      inside two clearance disks) the program fails at a building plane; that plane is then relaxed like a drone's, the
 *      building planes before it stay hard.
 *      status: 1 - pref, clipped to the ball, satisfies every plane and is the result; 2 - solved by the program;
 *      3 - no common point, the fallback's result.  slack: for status 3 the largest n . (point - v) over the drone
 *      planes at the result, not below 0; 0 for status 1 and 2.
 *   7. Ghost rows (counted handle, d >= counts[e]): out_vel 0 and every diagnostic 0 (status 0); the ghost's state is not
 *      read.
 * One workgroup per env, one lane per drone; a lane's planes live in a workspace the handle owns ([slot][6][E * N]
 * doubles, 2 * (max_neighbors + max_buildings) - 1 slots), allocated by the first call and grown by a call that needs
 * more: such a call allocates (and a growing one waits for the device), every other one is one launch without
 * allocation, synchronisation or atomics.  Calls on one handle must not overlap on different streams.
 * Every argument check runs before the first HIP call and a refused call writes nothing: RVO3D_ERR_STATE without a loaded
 * world, or for a motion without attached per-env sets; RVO3D_ERR_INVALID for a null args / out_vel / pointer inside
 * motion, for each non-finite or out-of-range double, for max_neighbors outside 1..16, max_buildings outside 0..8, and
 * for dt not finite or < 0 (checked with and without a motion). */
typedef struct rvo3d_orca_args {
  double time_horizon;                     /* finite > 0: tau                                              */
  double time_step;                        /* finite > 0: the step overlapping agents separate in (the env's: 1) */
  double max_speed, pref_speed;            /* finite >= 0                                                  */
  double neighbor_dist;                    /* finite > 0                                                   */
  int32_t max_neighbors, max_buildings;    /* 1..16, 0..8                                                  */
  double reach, below;                     /* building gate, finite > 0 / finite >= 0                      */
  double clear_xy;                         /* finite >= 0: extra clearance round the cylinder              */
  double *out_vel;                         /* DEVICE [E][N][3], required                                   */
  /* DEVICE [E][N], each nullable */
  int32_t *n_neighbors, *n_buildings, *status;
  double *slack;
} rvo3d_orca_args;
int rvo3d_orca_vel(rvo3d_env *h, const rvo3d_orca_args *args,
                   const rvo3d_building_motion *motion, double dt, void *stream);

/* The action whose kinematic step (drone.kinematicstep: rvo3d_step*) turns the handle's current velocity and heading
 * into the wanted velocity w = vel [E][N][3] f64 (DEVICE): action [E][N][3] f64 (DEVICE, may be vel itself),
 *   a0 = |w| - |v|,  a1 = wrap180(atan2(w_y, w_x) deg - yaw) / 90,  a2 = (asin(clamp(w_z / |w|, -1, 1)) deg - pitch) / 90,
 * |x| = sqrt((x_x*x_x + x_y*x_y) + x_z*x_z), deg = * 57.29577951308232, wrap180(t) = t - 360 * floor((t + 180) / 360);
 * |w| = 0 keeps both angles (a1 = a2 = 0).  Each component is then clipped to [-1, 1], as the step would clip it;
 * clipped (DEVICE [E][N] bytes, nullable): bit k set where component k needed it - the step then does not reach w.
 * Ghost rows (counted handle): zeros.  A finished drone is parked by the step whatever its action.  On a handle with
 * action_decimals >= 0 the step quantises the command like any action.  atan2 and asin are the device library's:
 * results agree with a host evaluation to a few ulp, not to the bit.  One launch, no synchronisation.
 * RVO3D_ERR_STATE without a loaded world, RVO3D_ERR_INVALID for a null vel / action. */
int rvo3d_vel_command(rvo3d_env *h, const double *vel, double *action, uint8_t *clipped, void *stream);

/* The action shield: ORCA as a safety filter behind any controller.  For every drone it takes the velocity the next
 * rvo3d_step would give the drone for `action`, and hands the action back untouched where that velocity satisfies
 * every ORCA plane of the current state; where it does not, the action is replaced by the command (rvo3d_vel_command)
 * for the permitted velocity nearest to it.  motion, dt: as for rvo3d_orca_vel.  Per live drone i of env e:
 *   S1. Preferred velocity: the velocity behind the step for this action, drone.kinematicstep in the step's own
 *       arithmetic (csrc/rvo3d_shield_rules.hpp: shield_pref is the statement):
 *         speed = max(0, |v| + clamp(a0, -1, 1)),  |v| = sqrt(fma(v_z, v_z, fma(v_y, v_y, v_x * v_x))),
 *         yaw' = np_mod(yaw + clamp(90 a1, -90, 90), 360),  pitch' = clamp(pitch + clamp(90 a2, -90, 90), -90, 90),
 *         (s_y, c_y) = sincos(yaw' * 0.017453292519943295), (s_p, c_p) likewise of pitch',
 *         pref = ((speed * c_p) * c_y, (speed * c_p) * s_y, speed * s_p).
 *       On a handle with action_decimals >= 0 the step quantises the action first; S1 predicts the unquantised one
 *       (evaluation handles use -1).
 *   S2. Planes: rules 2-5 of rvo3d_orca_vel on the current state, with one change: a neighbour whose dest flag is set
 *       takes no share - the step parks it whatever anyone commands - so the share against it is 1, not 0.5.
 *   S3. Program: rule 6 of rvo3d_orca_vel for the point of the ball |v| <= max_speed nearest pref: v, status, slack.
 *   S4. Identity where safe.  The row is intervened iff v != pref in some component.  Not intervened: the three doubles
 *       of out_action are the three doubles of action, bit for bit.  Intervened: out_action is rvo3d_vel_command's
 *       action for w = v on the drone's state.  flags: 8 for an intervened row, plus the command's clipped bits
 *       (1, 2, 4: component k was clipped, the step then does not reach v).  out_vel = v for every judged row.
 *   S5. Not judged - the action passes through, status, flags and slack are 0, pref_vel and out_vel are 0, the row
 *       enters no total: a drone whose dest flag is set (it still stands in the others' neighbour scans with the state
 *       on file); a row whose action has a non-finite component; a ghost row of a counted handle (its out_action is
 *       0, as rvo3d_vel_command writes ghosts; its state is not read).
 *   S6. totals (nullable, DEVICE [E][4] int64): the call ADDS to totals[e] the number of env e's rows that were judged,
 *       intervened, of status 3 (the fallback), and intervened with a clipped command.  The caller zeroes the array.
 * S2 and S3 are float64, rounded operation by operation, and defined to the last bit as rvo3d_orca_vel is, given pref.
 * S1 and the command go through the device library's sincos / atan2 / asin: against a host evaluation they agree to a
 * tolerance, not to the bit; against the step of the same device S1 is the same calls on the same inputs.
 * Limits.  A command that clips does not reach v.  Buildings are upright cylinders of unlimited height, as in
 * rvo3d_orca_vel.  The half share assumes that the other drone is shielded too.
 * One launch, no synchronisation and no atomics (one workgroup owns its env); the planes live in the workspace
 * rvo3d_orca_vel uses, allocated by the first call of either and grown by a call that needs more.  Calls on one handle
 * must not overlap on different streams.  Every argument check runs before the first HIP call and a refused call writes
 * nothing: the codes of rvo3d_orca_vel, RVO3D_ERR_INVALID also for a null action / out_action. */
typedef struct rvo3d_shield_args {
  double time_horizon;                     /* finite > 0: tau                                              */
  double time_step;                        /* finite > 0                                                   */
  double max_speed;                        /* finite >= 0                                                  */
  double neighbor_dist;                    /* finite > 0                                                   */
  int32_t max_neighbors, max_buildings;    /* 1..16, 0..8                                                  */
  double reach, below;                     /* building gate, finite > 0 / finite >= 0                      */
  double clear_xy;                         /* finite >= 0                                                  */
  const double *action;                    /* DEVICE [E][N][3], required                                   */
  double *out_action;                      /* DEVICE [E][N][3], required; may be action itself             */
  /* diagnostics, DEVICE, each nullable: [E][N][3] f64, [E][N][3] f64, [E][N] i32, [E][N] u8, [E][N] f64 */
  double *pref_vel, *out_vel;
  int32_t *status;
  uint8_t *flags;
  double *slack;
  int64_t *totals;                         /* DEVICE [E][4], nullable: judged, intervened, status 3, clipped */
} rvo3d_shield_args;
int rvo3d_shield_action(rvo3d_env *h, const rvo3d_shield_args *args,
                        const rvo3d_building_motion *motion, double dt, void *stream);

/* Zero-copy views of the state arrays, READ-ONLY: the step keeps values derived from the
 * state on file between calls (des_vel, the in-range words of the pair gate, the current /
 * previous waypoint); state is changed through rvo3d_set_state / rvo3d_reset*, which bring
 * them up to date or mark them stale. */
int rvo3d_state_ptrs(rvo3d_env *h, rvo3d_state_view *out);
/* Array-of-structs copies: pos/vel [E][N][3] f64, the rest [E][N]; any
 * pointer may be NULL.  set_state is for tests and checkpoint restore. */
int rvo3d_get_state(rvo3d_env *h, double *pos, double *vel, double *yaw, double *pitch,
                    double *real_len, double *max_dev, double *extra_len,
                    int32_t *wp_idx, uint8_t *arrive, uint8_t *dest, void *stream);
int rvo3d_set_state(rvo3d_env *h, const double *pos, const double *vel,
                    const double *yaw, const double *pitch, const double *real_len,
                    const double *max_dev, const double *extra_len,
                    const int32_t *wp_idx, const uint8_t *arrive, const uint8_t *dest,
                    void *stream);

/* Reads (and clears) the device error word into *flags (HOST).  Synchronises
 * the stream: opt-in, keep it out of the rollout loop. */
int rvo3d_error_flags(rvo3d_env *h, uint32_t *flags, void *stream);

/* Launch geometry chosen for this handle (diagnostics / bench):
 * threads per block, envs per block, blocks, dynamic LDS bytes. */
int rvo3d_launch_info(rvo3d_env *h, int32_t *threads, int32_t *envs_per_block,
                      int32_t *blocks, int32_t *lds_bytes);

/* The kernel instantiation this handle's calls launch, as rocprofv3 names it
 * ("rvo3d::env_kernel<MODE, NW, NFIX, TRAIN, PAD>"; mode 0 = rvo3d_observe, 1 = rvo3d_step,
 * 2 = rvo3d_step_autoreset / rvo3d_step_policy with autoreset), written to buf (HOST, cap bytes,
 * NUL-terminated): bench.py's roofline.kernel. */
int rvo3d_kernel_name(rvo3d_env *h, int32_t mode, char *buf, int32_t cap);

/* (Diagnostics - phase stamps, phase ablation - are not part of this library: they exist
 * only in the -DRVO3D_DIAG build that tools/ makes for itself, include/rvo3d_diag.h.) */

int rvo3d_version(void);
const char *rvo3d_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
