// rvo3d_step_body.hpp -- the body of the environment step kernels, as text.  NOT a header: rvo3d_step.hpp includes it
// once per kernel template (env_kernel, env_kernel_counted), inside the function's braces, with Pin, MODE, NW, NFIX,
// TRAIN, PAD, CNT and RVO3D_TWO_PHASE_ROWS in scope, and nothing else may include it (no include guard: it is meant to
// be included twice).  Text rather than a shared __device__ function: env_kernel's code has to stay exactly what it was
// before the counted kernels existed, and the body compiled as a function of its own and inlined does not give the
// same machine code (operand order, register numbers).
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Params P = Pin;
  // Inside the kernel P.N is the size of the RING the pair sweeps walk (neighbour d + k mod P.N) and of the
  // LDS layout; Nr is the number of drones an env really has.  They differ only in the padded compile-time
  // kernels (PAD): those take any N <= NFIX, the lanes d >= N of an env's segment are ghost drones parked at
  // infinity - never in range of anybody, never active - so envs of 33..63, 65..127, 129..255 (...) drones run
  // on the kernels whose index arithmetic folds (no generic-N spills; stage G shared between the lanes
  // at 128 / 256).
  static_assert(!PAD || NFIX != 0, "a padded kernel has a compile-time ring size");
  const int Nr = Pin.N;
  if (NFIX) { P.N = NFIX; P.epb = NFIX <= 64 ? 64 / NFIX : 1; }
  const int tid = threadIdx.x, T = (NW == 1 || NFIX) ? 64 * NW : (int)blockDim.x, N = P.N;
  const Lds L = carve_lds(smem, T, P.nm, P.epb, N, NW);
  const int el = tid / N;
  const int d = tid - el * N;
  const int e0 = blockIdx.x * P.epb;
  const int e = e0 + el;
  static_assert(!CNT || PAD, "per-env counts run on the padded kernels");
  // CNT: Nr stays the stride of every layout; the live drones of this lane's env are a number of its own (Nl), the
  // rows Nl <= d < Nr are ghosts that own rows of the outputs (ghost_in), written as zeros
  const int Nl = CNT ? (((el < P.epb) && (e < P.E)) ? live_count(P, e) : Nr) : Nr;
  const bool active = (el < P.epb) && (e < P.E) && (!PAD || d < Nl);
  const bool ghost_in = CNT ? ((el < P.epb) && (e < P.E) && d >= Nl && d < Nr) : false;
  const bool rowed = CNT ? (active || ghost_in) : active;  // has rows in the [E][N] layouts
  const int g = rowed ? e * (PAD ? Nr : N) + d : 0;
  const int lbase = el * N;
  const int full_rows = P.epb * (PAD ? Nr : N);                                            // rows of a full workgroup
  const int nrows = ((P.E - e0) < P.epb ? (P.E - e0) : P.epb) * (PAD ? Nr : N);            // rows of this workgroup
  const int row0 = e0 * (PAD ? Nr : N);
  const int lrow = PAD ? el * Nr + d : tid;  // this drone's row among the workgroup's rows (row writers)
  constexpr bool LITE = (MODE == kStepAutoReset);
  // stage G shared between the lanes (gate_words_shared): workgroups of exactly 64 NW drones
  constexpr bool GSH = NW > 1 && NFIX == 64 * NW;
  // stage X1 on the wave's compacted pair list (x1_queue): one-wave workgroups with a compile-time ring of 16 / 32 / 64
  constexpr bool XQ = NW == 1 && NFIX != 0;

  // Register discipline: values are loaded right before the phase that needs them and
  // stored as soon as they are final, so that across the sweeps little more than the
  // drone's own 8-value record and its action stay live (registers = waves per SIMD).
  RVO3D_STAMP(0);
  Drone S;
  S.x = S.y = S.z = S.vx = S.vy = S.vz = 0.0; S.r = 0.2; S.prio = 5;
  if (PAD && d >= Nl) {
    // a ghost: its fp64 record (restaged with everybody's below) sits at +inf - no exact test passes - and its
    // fp32 record, which stage_f32 never touches again, far outside every gate (1e30^2 overflows to +inf:
    // the sign test of stage G says "not in range"; never NaN against a real drone)
    S.x = S.y = S.z = __builtin_inf();
    const int o = el * 2 * N + d, os = el * N + d;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const float v = (k == WX || k == WY || k == WZ) ? 1e30f : (k == WKD ? -1.0f : 0.0f);
      if (k == WX || k == WY || k == WZ || k == WR) {
        L.w[k][o] = v;
        if (d <= (N >> 1)) L.w[k][o + N] = v;
      } else L.w[k][os] = v;
    }
  }
  double a[3] = {0, 0, 0}, cur[3] = {0, 0, 0}, dv[3] = {0, 0, 0};
  double dev = 0, max_dev = 0;
  int wpi = 1;

  // ---- phase 0: the drone's own record and its action; everything else about the pre-move
  //      state (waypoints, des_vel, deviation) is fetched after sweep A, which needs none of it
  uint32_t gw[NW];  // candidate words (stage G): on file from the previous step if it ended in this state
  const bool have_gw = MODE != kObserve && P.g_cached != 0;
  // the old count of this drone's row (clamp_kept), read before anything of this step is stored.  One-wave
  // workgroups read it here; several waves where the reset state is requested (one register less across the
  // sweeps: no spills there)
  uint32_t old_cnt = 0;
  // ONE batch of loads: old count, record, stage-G words, action - no address depends on a loaded value, and
  // nothing is computed from any of them before the last is requested (at the start of the kernel no other wave
  // has work to hide a round trip behind).  The action arrives as it was passed, in variables of its own per type:
  // a policy increment is float32, an absolute action float32 or float64.
  const bool act_f64 = P.action_mode != 1 && P.action_f64 != 0;
  float af[3] = {0.f, 0.f, 0.f};
  double ad[3] = {0, 0, 0};
  if (active) {
    if (LITE && NW == 1 && P.prev_cnt) old_cnt = (uint32_t)P.prev_cnt[g];  // raw: clamped where it is filed (clamp_kept)
    S.x = P.px()[g]; S.y = P.py()[g]; S.z = P.pz()[g];
    S.vx = P.vx()[g]; S.vy = P.vy()[g]; S.vz = P.vz()[g];
    if (P.uniform_rp) { S.r = P.r0; S.prio = P.prio0; }
    else { S.r = P.radius()[g]; S.prio = P.prio()[g]; }
    if (have_gw) {  // requested with the record: sweep A's stage X1 starts from them (no load behind the staging barrier)
#pragma unroll
      for (int w = 0; w < NW; ++w) gw[w] = P.gcache(w)[g];
    }
    if (MODE != kObserve) {
      if (act_f64) {
        const double* A = static_cast<const double*>(P.actions) + (size_t)g * 3;
        ad[0] = A[0]; ad[1] = A[1]; ad[2] = A[2];
      } else {
        const float* A = static_cast<const float*>(P.actions) + (size_t)g * 3;
        af[0] = A[0]; af[1] = A[1]; af[2] = A[2];
      }
      if (P.action_mode == 1) {
        // The trainer's glue (multi_ppo.py:196-205), in numpy's own types:
        //   a_inc = np.round(sample, 2)                  float32: rint(a * 100f) / 100f
        //   abs   = np.round(acceler * a_inc + vel, 2)   float32 product, widened, + float64
        const double vv[3] = {S.vx, S.vy, S.vz};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float r = __builtin_rintf(af[k] * 100.0f) / 100.0f;
          const double x = (double)(P.acceler * r) + vv[k];
          a[k] = __builtin_rint(x * 100.0) / 100.0;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) a[k] = act_f64 ? ad[k] : (double)af[k];
        const double act_scale = P.cold().act_scale;
        if (act_scale > 0) {
          a[0] = __builtin_rint(a[0] * act_scale) / act_scale;
          a[1] = __builtin_rint(a[1] * act_scale) / act_scale;
          a[2] = __builtin_rint(a[2] * act_scale) / act_scale;
        }
      }
    }
  }
  if (CNT && ghost_in && LITE && NW == 1 && P.prev_cnt) old_cnt = (uint32_t)P.prev_cnt[g];
  RVO3D_STAMP(1);
  double az[3] = {a[0], a[1], a[2]};  // action as the RVO code sees it (rvo_inter.py:118)
  if (norm3b(a[0], a[1], a[2]) < 1e-5) az[0] = az[1] = az[2] = 0.0;
  const double zero3[3] = {0, 0, 0};

  if (tid < P.epb) { L.any_reset[tid] = 0; L.far[tid] = 0; }
  if (LITE && NW > 1 && tid == 0) *L.any_old = 0;
  L.kept[tid] = 0;
  __syncthreads();  // flags zeroed before anyone raises them
  if (LITE && NW == 1 && rowed && P.prev_cnt) L.kept[lrow] = clamp_kept(P, old_cnt);  // until the rows are staged
  L.x[tid] = S.x; L.y[tid] = S.y; L.z[tid] = S.z;
  L.vx[tid] = S.vx; L.vy[tid] = S.vy; L.vz[tid] = S.vz;
  L.r[tid] = S.r; L.prio[tid] = S.prio;
  {
    const double p[3] = {S.x, S.y, S.z}, v[3] = {S.vx, S.vy, S.vz};
    stage_f32<NW>(P, L, el, d, active, p, v, az, S.r, S.prio);
  }
  __syncthreads();

  bool flag, collision = false;
  double tmin;

  if (MODE == kObserve) {
    if (active) {  // drone.dronestate (drone.py:254-263)
      double prev[3];
      max_dev = P.max_dev()[g];
      load3(P.cur(0), P.cur(1), P.cur(2), g, cur);
      load3(P.prev(0), P.prev(1), P.prev(2), g, prev);
      const double p[3] = {S.x, S.y, S.z};
      des_vel(P, p, cur, dv);
      dev = deviation(prev, cur, p);
      if (dev > max_dev) max_dev = dev;
    }
    const int kept = sweep_env<NW, true, true, TRAIN, GSH, XQ>(P, L, tid, el, d, g, active, S, zero3, true, true, flag,
                                               tmin, collision, gw, false);
    if (active) {
      write_vo_rows(P, L, tid, lbase, g, S, kept);
      if (P.zf16) stage_row(P, L, lrow, g, S, proprio_tail(dv, dev), kept);
      else {
        write_proprio(P, g, S, proprio_tail(dv, dev));
        publish_zero_run(P, g, kept);
        L.kept[lrow] = kept;
      }
      P.max_dev()[g] = max_dev;
      uint32_t dvk_a, dvk_b;
      dv_encode(dv, dvk_a, dvk_b);
      P.dvk_a()[g] = dvk_a; P.dvk_b()[g] = dvk_b;
#pragma unroll
      for (int w = 0; w < NW; ++w) P.gcache(w)[g] = gw[w];
    }
    if (CNT && ghost_in) ghost_row(P, L, lrow, g);
    __syncthreads();
    if (P.zf16) row_fill_pairs<NW>(P, L, tid, row0, nrows);
    else zero_fill(P, L, tid, row0, nrows);
    return;
  }

  RVO3D_STAMP(2);
  // ---- sweep A: ir_gym.rvo_reward_list_cal on the pre-move state (ir_gym.py:50-62)
  sweep_env<NW, false, false, TRAIN, GSH, XQ>(P, L, tid, el, d, g, active && !RVO3D_ABLATED(1), S, az, false, false, flag,
                              tmin, collision, gw, have_gw);
  // ---- everything else about this drone arrives in ONE batch of loads now (none of the
  //      addresses depends on a loaded value), then: drone.dronestate on the pre-move state
  //      (drone.py:254-263) and the RVO reward - the state is the one the previous step (or
  //      observe / reset) ended in, so its des_vel is on file and its deviation is already in
  //      max_deviation; only a state set from outside is recomputed - and
  //      drone.move_forward + kinematicstep (drone.py:96-129, 435-490), the post-move
  //      dronestate and the arrival flags of ir_gym.observation_reward (:168-193)
  double rew_k = 0;
  double mov_nc = 0;  // mov_reward (k form) if the step turns out collision-free
  bool f_dest = false;
  RVO3D_STAMP(3);
  // (the whole batch is issued here, ahead of the barrier below - a fence the compiler does not move
  // loads across: what the integration needs arrives while the RVO reward is being computed)
  // (up to 128 drones per env; at 256 the eighteen registers this keeps busy over the barrier cost more
  // than the latency they hide)
  constexpr bool kLoadAhead = NW <= 2;
  double prev[3] = {0, 0, 0}, yaw = 0, pitch = 0, real_len = 0, route_len = 0;
  int npts = 2;
  bool f_arrive_in = false, f_dest_in = false;
  if (active) {
    max_dev = P.max_dev()[g];
    load3(P.cur(0), P.cur(1), P.cur(2), g, cur);
    uint32_t dvk_a = 0, dvk_b = 0;
    if (P.dv_cached) { dvk_a = P.dvk_a()[g]; dvk_b = P.dvk_b()[g]; }
    if (kLoadAhead) {  // the integration state (the same ten loads behind the barrier otherwise)
      wpi = P.wp_idx()[g]; load3(P.prev(0), P.prev(1), P.prev(2), g, prev);
      yaw = P.yaw()[g]; pitch = P.pitch()[g]; real_len = P.real_len()[g]; route_len = P.route_len()[g];
      npts = P.n_points()[g]; f_arrive_in = P.arrive()[g] != 0; f_dest_in = P.dest()[g] != 0;
    }
    bool have = false;
    if (P.dv_cached) have = dv_decode(dvk_a, dvk_b, dv);
    if (!have) {
      if (!kLoadAhead) load3(P.prev(0), P.prev(1), P.prev(2), g, prev);
      const double p[3] = {S.x, S.y, S.z};
      des_vel(P, p, cur, dv);
      dev = deviation(prev, cur, p);
      if (dev > max_dev) max_dev = dev;
    }
    rew_k = rvo_reward_k(rvo_reward_pre(dv, a), flag, tmin);
  }
  RVO3D_STAMP(18);
  __syncthreads();  // everyone is done with the pre-move LDS image
  if (active) {
    if (!kLoadAhead) {
      wpi = P.wp_idx()[g]; load3(P.prev(0), P.prev(1), P.prev(2), g, prev);
      yaw = P.yaw()[g]; pitch = P.pitch()[g]; real_len = P.real_len()[g]; route_len = P.route_len()[g];
      npts = P.n_points()[g]; f_arrive_in = P.arrive()[g] != 0; f_dest_in = P.dest()[g] != 0;
    }
    // extra_len is only ever WRITTEN by the step (drone.py:188, ir_gym.py:176): not loaded, and
    // stored only by the drones that set it; wp_idx / arrive / dest likewise only when they change
    bool ex_set = false;
    double extra_len = 0.0;
    const int wpi_in = wpi;
    bool f_arrive = f_arrive_in;
    f_dest = f_dest_in;

    double speed = norm3b(S.vx, S.vy, S.vz);
    const double acc = clampd(a[0] * 1.0, -1.0, 1.0);
    const double dyaw = clampd(a[1] * 90.0, -90.0, 90.0);
    const double dpit = clampd(a[2] * 90.0, -90.0, 90.0);
    const double nv = speed + acc;
    speed = (0.0 > nv) ? 0.0 : nv;
    yaw = np_mod(yaw + dyaw, 360.0);
    pitch = clampd(pitch + dpit, -90.0, 90.0);
    double nvx = 0.0, nvy = 0.0, nvz = 0.0;
    if (!f_dest) {  // `stop` := map_size (env_base.py:142, drone.py:107): parked once finished
      double sy, cy, sp, cp;
      sincos(yaw * kDeg2Rad, &sy, &cy);
      sincos(pitch * kDeg2Rad, &sp, &cp);
      nvx = speed * cp * cy; nvy = speed * cp * sy; nvz = speed * sp;
    }
    const double q0 = S.x, q1 = S.y, q2 = S.z;
    S.x = S.x + nvx; S.y = S.y + nvy; S.z = S.z + nvz;
    S.vx = nvx; S.vy = nvy; S.vz = nvz;
    real_len = real_len + norm3b(S.x - q0, S.y - q1, S.z - q2);
    const double p[3] = {S.x, S.y, S.z};
    const double T04 = P.cold().T04;  // one read for the arrival tests and des_vel below (rvo3d_math.hpp)
    // the destination matters only next to a waypoint: fetched on demand (rare)
    double dst[3] = {0, 0, 0};
    if (f_arrive || arrived(T04, p, cur)) load_wp(P, g, npts - 1, dst);
    if (arrived(T04, p, cur)) {  // drone.py:116-129
      const bool at_dst = arrived(T04, p, dst);
      if (at_dst) { extra_len = real_len - route_len; ex_set = true; }  // destination_arrive side effect
      if (!at_dst && wpi < npts - 1) {
        wpi += 1;
        prev[0] = cur[0]; prev[1] = cur[1]; prev[2] = cur[2];
        load_wp(P, g, wpi, cur);
        store3(P.cur(0), P.cur(1), P.cur(2), g, cur);
        store3(P.prev(0), P.prev(1), P.prev(2), g, prev);
        f_arrive = false;
      }
    }
    // dronestate on the post-move state
    des_vel(T04, p, cur, dv);
    dev = deviation(prev, cur, p);
    if (dev > max_dev) max_dev = dev;
    // arrival flags (ir_gym.py:168-181)
    bool arrive_r = false, dest_r = false;
    const int waypoint_num = wpi;
    if (!f_arrive && arrived(T04, p, cur)) { f_arrive = true; arrive_r = true; }
    if (f_arrive) {
      if (arrived(T04, p, dst)) {
        extra_len = real_len - route_len;
        ex_set = true;
        if (!f_dest) { f_dest = true; dest_r = true; }
      }
    }
    const double exlen = real_len - route_len + 4;
    mov_nc = mov_reward_k(P, false, arrive_r, waypoint_num, npts - 1, dest_r, dev, exlen > 0,
                          exlen);
    RVO3D_STAMP(19);
    // the map's bounds are launch constants: read once, here, ahead of the step's first store (scalar loads) - and
    // tested with `|`: `||` made each bound a lane-predicated vector load with a round trip of its own
    const double map_x = P.cold().map[0], map_y = P.cold().map[1], map_z = P.cold().map[2];
    collision = building_hit(P, S, e);
    if ((S.x < 0) | (S.x > map_x) | (S.y < 0) | (S.y > map_y) | (S.z < 0) | (S.z > map_z))
      collision = true;  // drone.drone_out_map, drone.py:213-225
    // final for this step unless the drone is reset below
    P.yaw()[g] = yaw; P.pitch()[g] = pitch; P.real_len()[g] = real_len;
    if (ex_set) P.extra_len()[g] = extra_len;
    if (wpi != wpi_in) P.wp_idx()[g] = wpi;
    if (f_arrive != f_arrive_in) P.arrive()[g] = f_arrive ? 1 : 0;
    if (f_dest != f_dest_in) P.dest()[g] = f_dest ? 1 : 0;
    P.info[g] = f_arrive ? 1 : 0;
    P.finish[g] = f_dest ? 1 : 0;
  }
  L.x[tid] = S.x; L.y[tid] = S.y; L.z[tid] = S.z;
  L.vx[tid] = S.vx; L.vy[tid] = S.vy; L.vz[tid] = S.vz;
  {
    const double p[3] = {S.x, S.y, S.z}, v[3] = {S.vx, S.vy, S.vz};
    stage_f32<NW>(P, L, el, d, active, p, v, az, S.r, S.prio);
  }
  __syncthreads();

  RVO3D_STAMP(4);
  // ---- sweep B: the pair part of ir_gym.observation_reward (ir_gym.py:197).
  // In the fused auto-reset step an env that resets discards the step's VO rows (its
  // observation is recomputed after the reset), so a collision-only sweep runs first,
  // the resets are settled, and then ONE sweep produces the rows - on the post-move
  // state with the action, or on the post-reset state with action 0.
  int kept = 0;
  if (LITE) {
    if (collide_env<NW, TRAIN, GSH>(P, L, tid, el, d, active && !RVO3D_ABLATED(2), S, gw)) collision = true;
  } else {
    kept = sweep_env<NW, true, true, TRAIN, GSH, XQ>(P, L, tid, el, d, g, active && !RVO3D_ABLATED(2), S, az, false,
                                     false, flag, tmin, collision, gw, false);
  }
  bool do_reset = false;
  if (active) {
    const double rew64 = k_over_1000(rew_k) + k_over_1000(collision ? -50000.0 : mov_nc);  // mdin.py:28
    P.reward[g] = (float)rew64;
    if (P.reward64) P.reward64[g] = rew64;
    P.done[g] = collision ? 1 : 0;
    do_reset = LITE && (collision || f_dest);
  }
  if (CNT && ghost_in) ghost_outputs(P, g, LITE);

  RVO3D_STAMP(5);
  if (LITE) {
    if (active && P.reset_mask) P.reset_mask[g] = do_reset ? 1 : 0;
    if (do_reset) L.any_reset[el] = 1;
    __syncthreads();  // sweep reads done; any_reset visible
    // the reset drones' start state is requested first; then - the workgroup's early zero blocks
    // (two-phase row writer: every 64-B block without proprio bytes) are stored, which takes a
    // few thousand cycles of store issue and needs no data at all: the loads land meanwhile
    double p[3] = {0, 0, 0}, rcur[3] = {0, 0, 0}, rdev = 0.0;
    uint32_t rdv_a = 0, rdv_b = 0;
    // (see phase 0; requested in one batch with the start state, filed behind it; visible to early_zero_blocks
    // behind the next barrier)
    if (NW > 1 && rowed && P.prev_cnt) old_cnt = (uint32_t)P.prev_cnt[g];
    if (do_reset) {  // (dronestate of the start state: static, tabulated by rvo3d_load_world, dv0_kernel)
      load_wp(P, g, 0, p);
      rdev = P.dev0()[g];
      load_wp(P, g, 1, rcur);
      rdv_a = P.dv0_a()[g]; rdv_b = P.dv0_b()[g];
    }
    if (NW > 1 && rowed && P.prev_cnt) {
      L.kept[lrow] = clamp_kept(P, old_cnt);
      if (old_cnt != 0) *L.any_old = 1;
    }
    RVO3D_STAMP(26);
    // (one-wave workgroups: 64 x 4096 -2 %; with several waves per workgroup the blocks go out right
    // before the rows sweep instead, which measured better there)
    if (NW == 1 && RVO3D_TWO_PHASE_ROWS && !RVO3D_ABLATED(16)) early_zero_blocks<NW>(P, L, tid, row0, nrows);
    RVO3D_STAMP(27);
    if (do_reset) {  // drone.reset (drone.py:270-291); extra_len survives
      // (read here, not inside the rare branch below: a Cold read under a lane-dependent condition turns the
      // restage's reads of cen[] / cmax into vector loads, which queue behind the twelve stores of this block)
      const double T04r = P.cold().T04;
      S.x = p[0]; S.y = p[1]; S.z = p[2]; S.vx = S.vy = S.vz = 0.0;
      dev = rdev;
      cur[0] = rcur[0]; cur[1] = rcur[1]; cur[2] = rcur[2];
      if (!dv_decode(rdv_a, rdv_b, dv)) {
        des_vel(T04r, p, cur, dv);
        dev = deviation(p, cur, p);  // previous_des = waypoints[0] = the start position
      }
      store3(P.cur(0), P.cur(1), P.cur(2), g, cur);
      store3(P.prev(0), P.prev(1), P.prev(2), g, p);
      max_dev = dev > 0.0 ? dev : 0.0;
      P.wp_idx()[g] = 1; P.arrive()[g] = 0; P.dest()[g] = 0;
      P.real_len()[g] = 0.0; P.yaw()[g] = 0.0; P.pitch()[g] = 0.0;
      L.x[tid] = S.x; L.y[tid] = S.y; L.z[tid] = S.z;
      L.vx[tid] = 0.0; L.vy[tid] = 0.0; L.vz[tid] = 0.0;
      const double v0[3] = {0, 0, 0};
      stage_f32<NW>(P, L, el, d, true, p, v0, az, S.r, S.prio);
    }
    // an env that reset somebody is observed with action 0 (ir_gym.py:372-383): its drones zero the
    // fp32 copy of their action now (any_reset is visible since the barrier above; the rows sweep is
    // behind the next one), so stage X1 needs no per-trip "action or zero" selects
    if (active && L.any_reset[el] != 0) {
      const int os = el * N + d;
      L.w[WAX][os] = 0.f; L.w[WAY][os] = 0.f; L.w[WAZ][os] = 0.f;
    }
  }
  // everything about this drone except its VO rows is final now.  The stores wait until
  // after the last sweep (vector memory returns in order: a load behind a store waits for
  // it, and measured: stores issued here cost 1.5 %); the drone's record and the rounded
  // floats of des_vel / deviation stay live across the sweep.
  if (active) {
    uint32_t dvk_a, dvk_b;
    dv_encode(dv, dvk_a, dvk_b);  // des_vel, on file for the next step
    P.dvk_a()[g] = dvk_a; P.dvk_b()[g] = dvk_b;
  }
  const ProprioTail ptail = proprio_tail(dv, dev);
  // max_deviation is final as well; stored here - unlike the rest of the record - because two
  // registers less across the sweep are worth more than the store costs (config 5: -1.5 %)
  if (active) P.max_dev()[g] = max_dev;
  if (LITE) {
    __syncthreads();
    RVO3D_STAMP(6);
    // rows for every env: ir_gym.observation_reward's VO part (the env kept its state) or
    // ir_gym.env_observation with action 0 (the env reset a drone, ir_gym.py:372-383)
    // (ghost lanes of a padded env follow their env: the shared stage G below needs every lane, and its
    // barrier every wave)
    const bool env_reset = (active || (PAD && el < P.epb)) && (L.any_reset[el] != 0);
    bool c2 = false;
    const double aa[3] = {env_reset ? 0.0 : az[0], env_reset ? 0.0 : az[1], env_reset ? 0.0 : az[2]};
    // stage G: the collision sweep delivered the words of the post-move state; only pairs
    // with a reset drone changed since (larger envs: recompute when the env reset anyone)
    bool have_gw2 = !env_reset;
    if (NW == 1) {
      const unsigned long long rlanes = __ballot(do_reset);
      if (L.far[el] != 0) {
        uint32_t valid[1];
        valid_offsets<1>(N, d, valid);
        gw[0] = valid[0];
      } else {
        gw[0] = regate_resets(P, L, tid, el, d, active, rlanes, gw[0]);
      }
      have_gw2 = true;
    }
    if (RVO3D_ABLATED(2)) have_gw2 = false;  // diagnostics: the collision sweep was skipped
    if (NW > 1 && RVO3D_TWO_PHASE_ROWS && !RVO3D_ABLATED(16)) early_zero_blocks<NW>(P, L, tid, row0, nrows);
    kept = sweep_env<NW, true, false, TRAIN, GSH, XQ>(P, L, tid, el, d, g, active && !RVO3D_ABLATED(4), S, aa,
                                      false, env_reset, flag, tmin, c2, gw, have_gw2);
  }
  RVO3D_STAMP(7);
  // kept rows first (their loads from the row scratch would otherwise queue behind the fill's
  // stores); then every other byte of the rows - proprio and zeros - in coalesced 16-B stores
  // (a lane writing its own 48 proprio bytes costs as much as the whole zero fill: 64 rows =
  // 64 partial cache lines per store instruction); the state stores drain behind them.
  const bool two_phase = LITE && RVO3D_TWO_PHASE_ROWS;
  if (NW > 1 && two_phase) {  // every wave's early zeros have landed before any wave writes kept rows
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (active) {
    if (!RVO3D_ABLATED(8)) {
      // kept rows go over zeros this wave (or, before the sweep's barrier, this workgroup)
      // stored earlier: those stores have to have landed
      if (two_phase) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      write_vo_rows(P, L, tid, lbase, g, S, kept);
      RVO3D_STAMP(16);
      if (P.zf16) stage_row(P, L, lrow, g, S, ptail, kept);
      else { write_proprio(P, g, S, ptail); publish_zero_run(P, g, kept); }
    }
    if (!P.zf16) L.kept[lrow] = kept;
  }
  if (CNT && ghost_in) ghost_row(P, L, lrow, g);
  __syncthreads();  // the staged rows / L.kept complete
  RVO3D_STAMP(17);
  if (!RVO3D_ABLATED(16)) {
    if (two_phase) late_row_windows<NW>(P, L, tid, row0, nrows);
    else if (P.zf16) row_fill_pairs<NW>(P, L, tid, row0, nrows);
    else zero_fill(P, L, tid, row0, nrows);
  }
  RVO3D_STAMP(8);
  if (active) {
#pragma unroll
    for (int w = 0; w < NW; ++w) P.gcache(w)[g] = gw[w];
    P.px()[g] = S.x; P.py()[g] = S.y; P.pz()[g] = S.z;
    P.vx()[g] = S.vx; P.vy()[g] = S.vy; P.vz()[g] = S.vz;
  }
  RVO3D_STAMP(9);
