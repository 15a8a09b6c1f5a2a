/* omnisafe_amd_env.h -- a device env of your own: the description contract and the C ABI of the library that
 * omnisafe_amd.build.build_custom_env(header, struct) makes of it (csrc/custom/custom_env.hip).  libomnisafe_amd.so
 * exports none of these symbols; every custom library exports all of them.  Error codes are omnisafe_amd.h's.
 *
 * THE DESCRIPTION is a struct of static members in a header of yours.  The header is compiled for gfx950 behind
 * csrc/env_device.h, inside a `#pragma clang fp contract(off)` region: float32, no fused multiply-adds.
 *
 *   struct MyEnv {
 *     static constexpr int STATE = ..;     // floats per row of the (N, STATE) state matrix, 1 .. 64 (1 .. 256 with
 *                                          // LDS_ROW = true)
 *     static constexpr int OBS = ..;       // observation columns, >= 1
 *     static constexpr int DYN = ..;       // leading state floats a transition changes (<= STATE; with LDS_ROW the
 *                                          // columns [DYN, STATE) are the objects, see OBJECT ROWS below)
 *     static constexpr int ACT = ..;       // action columns, 1 .. 32
 *     static constexpr int TRACE = ..;     // leading state floats in an evaluator trace record, <= STATE
 *     static constexpr bool LDS_ROW = false;  // false: the state of an env is what load() puts into Regs; true: the
 *                                          // row also holds objects, kept in LDS (OBJECT ROWS below)
 *     static constexpr int LEVELS = ..;    // optional: the highest level, 0 .. 2 (default 2)
 *     static constexpr int LANES = ..;     // optional: lanes per env in the per-step kernel, 16 / 32 / 64 (default 32)
 *     static __device__ float fresh_obj(const OsaEnvAt&, int col);    // with LDS_ROW: object column col of a fresh row
 *     struct Regs { ... };                 // an aggregate: the registers that hold a state row
 *     static __device__ void load(Regs&, const float* srow);          // from the env's row of the state matrix
 *     static __device__ void store(const Regs&, float* srow);         // and back (one lane per env calls it)
 *     static __device__ void fresh(Regs&, const OsaEnvAt&, const float* row);   // the state after a reset
 *     static __device__ void transition(Regs&, const float* row, const OsaEnvAt&, float a0, float a1,
 *                                       float& reward, float& cost);  // ACT <= 2: the action columns (ACT = 1:
 *                                                                     // a1 is 0, no second column is read), or
 *     static __device__ void transition(Regs&, const float* row, const OsaEnvAt&, const float* act,
 *                                       float& reward, float& cost);  // any ACT: the env's action row, act[0 .. ACT)
 *     static __device__ float obs_col(const Regs&, const float* row, int level, int col);   // 0 for col >= OBS
 *     static __device__ float state_col(const Regs&, const float* row, int col);            // col < TRACE
 *     static __device__ bool terminal(const Regs&, const float* row, const OsaEnvAt&);      // optional: true ends
 *                                                                     // the episode (see TERMINATION below)
 *     static constexpr float DRAW_VIEW = ..;    // optional, with draw(): half-width of the fixed camera's view, > 0
 *     static constexpr float DRAW_TRACK = ..;   // optional: half-width of the tracking camera's view (default 1)
 *     static __device__ void position(const float* rec, float& x, float& y);   // with draw(): what the trail and
 *                                                                     // the tracking camera follow
 *     static __device__ void draw(const float* rec, const OsaDrawAt&, OsaScene&);           // optional: the picture
 *                                                                     // of a state row (see DRAWING below)
 *     static constexpr int PARAMS = P;                        // optional: P runtime parameters, 1 .. 16, and with it
 *     static constexpr float PARAM_DEFAULT[P] = {..};         //   their values where the caller names none,
 *     static constexpr const char* PARAM_NAMES[P] = {..};     //   their names (env_cfgs keys), and
 *     static __device__ void bind(Regs&, const float* par);   //   what puts them into Regs (see PARAMETERS below)
 *   };
 *
 * `row` is nullptr for a description with LDS_ROW = false, in every kernel: its state is its Regs.  With LDS_ROW = true
 * it is the env's row in LDS, never nullptr (OBJECT ROWS below).  Actions arrive unclamped.  OsaEnvAt {seed, pos, n, level, cost_p} says where
 * the call stands: env index n at position pos of the Philox stream `seed`; draw with
 * osa_philox(seed ^ MY_KEY, pos, ((unsigned long long)n << 20) + block, w) and osa_u01(w[i]) so that the per-step
 * launches (pos = 0 for the reset, then 1, 2, ...) and the evaluation kernel (episode k = env index k) play the same
 * episodes.  fresh() of a truncating step and the transition of the same step see the same pos.  Every lane of an
 * env runs load / transition / terminal / fresh with the same inputs, so they must be deterministic functions of their
 * arguments: no atomics, no cross-lane operations, no memory but the arguments.
 *
 * OBJECT ROWS.  A description with LDS_ROW = true has a field of objects that a lidar and a cost loop walk: hazards,
 * buttons, obstacles.  Its state row has up to 256 floats, of which the leading DYN are what a transition changes --
 * what load() and store() move between the row and Regs -- and the columns [DYN, STATE) are the objects.
 *   - The objects are written only at a reset, one call fresh_obj(at, col) per column col in [DYN, STATE), by many lanes
 *     at once; between resets they are read-only.  fresh_obj is a function of (at, col) alone: it does not see the
 *     runtime parameters of a description with PARAMS (they are bound into Regs, and fresh_obj gets none).
 *   - fresh() is called after the fresh objects are in `row` and may read them (the Goal family places its goal away
 *     from the fresh hazards this way).
 *   - Every member that takes `const float* row` (load, fresh, transition, terminal, obs_col, state_col) gets the env's
 *     row in LDS.  Only its columns [DYN, STATE) mean anything outside load(): the leading DYN floats are the Regs, and
 *     the row's copy of them is stale or unwritten.  load() alone is handed a row whose leading floats are the stored
 *     state (the per-step kernel stages the whole row first; the persistent players never call load()).
 *   - An object may move between resets only as a closed form of the Regs (an episode step count kept in a DYN column
 *     and a phase in the object's read-only columns, say): the cost, the lidar and draw() compute where it stands.
 *   - state_col(col) must give what store() and fresh_obj() leave in column col of the state matrix for col < TRACE, as
 *     for any description; read the object columns from `row`.
 *   - terminal(), draw() with position() and DRAW_VIEW, and PARAMS with bind() combine with LDS_ROW = true exactly as
 *     they do with register state; draw() reads the objects from `rec` (TRACE must reach them).
 *   - The per-step kernel is osa_custom_row_env_kernel (csrc/env_frame.h): LANES lanes per env and 64 / LANES envs per
 *     workgroup, each with a slice of STATE floats in LDS; the order inside a step is that of PARAMETERS below with
 *     "the fresh objects" between the redraw and fresh().  OsaNavEnv<OsaPoint, OsaGoal> and OsaNavEnv<OsaCar, OsaGoal>
 *     (csrc/env_device.h) are valid descriptions of this kind as they stand; tests/custom_envs/button.h is a task
 *     written from scratch on the same robots.
 *   - The persistent players keep 16 rows per workgroup in LDS behind their own buffers and return OSA_EUNSUPPORTED
 *     where that passes 64 KB: with STATE = 256 the evaluation takes policy inputs up to 736 columns, the collection
 *     observations up to 234.
 *
 * TERMINATION.  Every env counts the steps of its episode (steps[n]) and truncates when the count reaches `horizon`.
 * A description without terminal() never ends an episode otherwise, so its envs truncate together every `horizon`
 * steps after a common reset.  One with terminal() is asked once per step, after transition(), on the post-transition
 * state and with the OsaEnvAt of that transition; true ends the episode of that env alone:
 *   - the step reports terminated = 1, truncated = 0 and the reward and cost of that transition; termination wins
 *     over a time limit reached on the same step;
 *   - the env is reset by fresh() at the same stream position, exactly as on a truncating step;
 *   - final_obs is NOT written for a terminating env (only truncated paths are bootstrapped from it);
 *   - a step truncates when steps[n] + 1 >= horizon and it is not terminal; steps[n] returns to 0 on either end.
 * The evaluation kernel ends episode k on the same answer, with ep_len the steps played.
 *
 * COLLECTION.  osa_custom_collect_episodes (OfflineDataCollector) plays the description in lanes that run episode after
 * episode inside one launch.  It calls the same members in the same order as the per-step kernel -- transition(),
 * terminal(), obs_col() on the post-transition state, then on an ending step fresh() at the step's own OsaEnvAt and
 * obs_col() on the fresh state -- so a description needs nothing new for it; obs_col() is called for every column of
 * the row whether or not the episode ends, and the rows it gives are stored raw.
 *
 * PARAMETERS.  A description with PARAMS computes with P floats that are no compile-time constants: every env has a
 * row of them, drawn anew for each of its episodes.
 *   - The caller gives every parameter a range (lo, hi), both float32, in a (2, P) device array `range` (lo = range[k],
 *     hi = range[P + k]); lo == hi fixes the parameter.  The kernels read the array through its pointer at every reset,
 *     so a change takes effect at each env's next reset -- also under a captured graph that keeps replaying.
 *   - The rows live in a matrix par[N][ld_par] (ld_par >= P) of their own, not in the state: STATE, store() and trace
 *     records are what they are without PARAMS.
 *   - At every reset of env n at stream position pos -- the common reset, a truncation, a terminal() end -- the row is
 *     redrawn before fresh(): parameter k from word k & 3 of osa_philox(seed ^ OSA_PARAM_KEY, pos, (n << 20) + (k >> 2))
 *     with OSA_PARAM_KEY = 0x8CB92BA72F3D8DD7 (csrc/env_params.h), u = osa_u01(word), and without fused multiply-adds
 *         span = hi - lo;  add = span * u;  v = fminf(lo + add, hi)
 *     so lo == hi gives exactly lo and no value leaves [lo, hi].
 *   - bind(s, par) copies what the description needs of par[0 .. P) into members of its Regs; every other member then
 *     sees the parameters through Regs, its signature unchanged.  A kernel calls it after load() and again after a
 *     redraw; load() and fresh() must leave alone the members that bind() sets.
 *   - The order inside a step: load, bind; transition, terminal; on a truncating step final_obs (still under the ended
 *     episode's parameters); on a reset the redraw, bind, fresh; the observation; one lane writes the redrawn row.
 *   - The two persistent players keep the row in registers and redraw it at every in-kernel reset, at the ending
 *     step's position like fresh(); the evaluation kernel also leaves each episode's row in a (K, P) output.
 *   - PARAM_NAMES are the keys a caller names the parameters by (make(env_id, wind=0.3, band=(0.4, 0.8)), env_cfgs,
 *     set_param): identifiers, distinct, and neither `horizon` nor `seed`.
 *   - draw() gets the row of the episode it draws as OsaDrawAt::par (nullptr without PARAMS).
 * The plain entry points of a library with PARAMS return OSA_EUNSUPPORTED (they would run with unbound parameters), and
 * so do the parameter-taking ones of a library without; every library has both sets.
 *
 * DRAWING.  A description with draw() can be looked at: osa_custom_render_episode rasterises frames of its state rows
 * (csrc/scene_render.h), which Evaluator.render, Agent.render, AgentGroup.render and the env's render() call.  Without
 * the member the description "does not draw": osa_custom_render_episode returns OSA_EUNSUPPORTED, and nothing else
 * about the library differs.
 *   - `rec` is the TRACE leading floats of a state row: in a replay the tail of a trace record, in env.render() the
 *     leading floats of the env's row of the state matrix.  These are the same floats (state_col(col) of a traced
 *     state is srow[col] of the stored one for col < TRACE); the per-step evaluator path relies on that already.
 *     draw() and position() may read rec[0 .. TRACE) and nothing else.
 *   - OsaDrawAt {int level; int hit; int frame; const float* par;}: the level the caller names, the caller's
 *     hit[f] != 0 (the evaluator: the step into this record had a positive cost), the record's index f, and the P
 *     parameters of the episode the record is of (PARAMETERS above; nullptr for a description without PARAMS).
 *   - draw() paints by appending primitives to the scene in painter's order (a later primitive wins); a frame starts
 *     as the background everywhere (OSA_COLOUR_OUTSIDE).  Each test is float32 without fused multiply-adds, on the
 *     sub-sample (x, y) with dx = x - ox, dy = y - oy:
 *         scene.disc(ox, oy, r2, colour)             dx*dx + dy*dy <= r2
 *         scene.ring(ox, oy, lo2, hi2, colour)       lo2 <= dx*dx + dy*dy && dx*dx + dy*dy <= hi2
 *         scene.box(x0, y0, x1, y1, colour)          x0 <= x && x <= x1 && y0 <= y && y <= y1
 *         scene.segment(ax, ay, bx, by, hw2, colour) the segment test of osa_render_episode (omnisafe_amd.h) with
 *                                                    e = b - a and L2 = ex*ex + ey*ey, computed once when staged
 *         scene.trail(hw2, colour)                   at most once (a second call is ignored): the path through
 *                                                    position() of records max(0, f - trail) .. f, segment by segment
 *                                                    at half-width sqrt(hw2), is painted at this place in the order;
 *                                                    never called: no trail
 *   - A colour is 0xRRGGBB.  The palette of osa_render_episode is there by name: OSA_COLOUR_OUTSIDE, _FLOOR, _COST,
 *     _RING, _HAZARD, _GOAL, _VASE, _TRAIL, _POINT, _CAR, _HIT, _HEADING.
 *   - A scene holds at most OSA_DRAW_MAX = 64 primitives (the trail is one); what is appended past the cap is
 *     dropped.  osa_custom_render_info reports the cap.
 *   - The sub-sample positions, the integer mean per channel, the cameras, first / count / trail / hit and the
 *     argument checks are those of osa_render_episode (omnisafe_amd.h) and are not restated here.  Only the centre
 *     and the half-width of the view differ: the fixed camera looks at (0, 0) with half-width DRAW_VIEW, the tracking
 *     camera at position() of the frame's record with half-width DRAW_TRACK.
 *   - draw() runs in one lane per workgroup, position() in many; both must be deterministic functions of `rec` (and
 *     `at`): no atomics, no cross-lane operations, no memory but the arguments.
 *
 * A static_assert with a message that names the member rejects LDS_ROW == true without fresh_obj, a member named
 * fresh_obj that cannot be called as stated above (with LDS_ROW == true), STATE outside 1 .. 64 (outside 1 .. 256 with
 * LDS_ROW == true), DYN > STATE, ACT outside 1 .. 32, TRACE > STATE, a missing member, and a member named terminal that cannot be called as stated above (it
 * would silently be an env that never ends), and likewise a member named draw that cannot be called as stated above,
 * draw without position or without DRAW_VIEW, DRAW_VIEW <= 0, and draw with TRACE == 0; PARAMS outside 1 .. 16, PARAMS
 * without bind, PARAM_DEFAULT or PARAM_NAMES, either array with another length than PARAMS, a member named bind that
 * cannot be called as stated above, and names that are no identifiers, repeat, or are `horizon` or `seed`.  A
 * description without PARAMS is compiled as if none of this existed.
 */
#ifndef OMNISAFE_AMD_ENV_H
#define OMNISAFE_AMD_ENV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* out[0 .. 8) = STATE, OBS, DYN, ACT, TRACE, LEVELS (the highest level), LANES, and 1 where the description has
 * terminal() (else 0).  The Python side reads every dimension from here. */
int osa_custom_env_info(int out[8]);

/* The row kind: out[0 .. 4) = 1 where the description has LDS_ROW = true (else 0), the widest STATE of that kind (256 or
 * 64), and two reserved 0. */
int osa_custom_row_info(int out[4]);

/* One reset (reset_only != 0) or one step of N envs: the argument list and the semantics of osa_nav_env_step
 * (omnisafe_amd.h).  state is (N, STATE) float32, action (N, >= ACT) with row stride ld_action, obs (N, obs_dim >= OBS)
 * with row stride ld_obs; columns OBS .. obs_dim are written as zeros.  level: 0 .. LEVELS. */
int osa_custom_env_step(unsigned long long seed, unsigned long long step, const unsigned long long* step_base, int N,
                        int obs_dim, int horizon, int level, float* state, int* steps, const float* action,
                        int ld_action, float* obs, int ld_obs, float* reward, float* cost, uint8_t* terminated,
                        uint8_t* truncated, float* final_obs, int ld_final, int reset_only, void* stream);

/* K evaluation episodes in one launch: the argument list and the semantics of osa_eval_episodes (omnisafe_amd.h) with
 * the level in the place of env_kind.  A trace record holds obs_dim (+ 1 with saute) + act_dim + 3 + TRACE floats. */
int osa_custom_eval_episodes(int level, int K, int obs_dim, int act_dim, int hidden, const float* params,
                             const float* norm_mean, const float* norm_std, const long* norm_count, float norm_clip,
                             const float* old_min, const float* old_max, float min_action, float max_action,
                             unsigned long long seed, int horizon, float cost_p, int max_steps, int saute,
                             float saute_budget, float saute_gamma, int early_terminated, double cost_limit,
                             double cost_criteria, double* ep_ret, double* ep_cost, int* ep_len, float* trace,
                             void* stream);

/* One agent's block of dataset rows in one launch: the argument list and the semantics of osa_collect_episodes
 * (omnisafe_amd.h) with the level in the place of env_kind.  A description with terminal() ends episodes per lane: the
 * terminating step's row carries done = 1 and the post-transition observation as next_obs, and the lane is reset by
 * fresh() at the same stream position (see COLLECTION above). */
int osa_custom_collect_episodes(int level, int K, int rows_per_lane, long total_rows, int obs_dim, int act_dim,
                                int hidden, const float* params, const float* norm_mean, const float* norm_std,
                                const long* norm_count, float norm_clip, const float* old_min, const float* old_max,
                                float min_action, float max_action, unsigned long long seed,
                                unsigned long long noise_seed, int horizon, float cost_p, float* obs, int ld_obs,
                                float* action, int ld_act, float* reward, float* cost, float* next_obs, int ld_next,
                                float* done, double* ep_ret_sum, double* ep_cost_sum, int* ep_count, void* stream);

/* What the description says about drawing: out_i[0 .. 4) = 1 where it has draw() (else 0), OSA_DRAW_MAX, TRACE, and a
 * reserved 0; out_f[0 .. 2) = DRAW_VIEW, DRAW_TRACK (both 0 where it does not draw). */
int osa_custom_render_info(int out_i[4], float out_f[2]);

/* Frames first .. first + count - 1 of one episode, as osa_render_episode (omnisafe_amd.h) with the level in the place
 * of env_kind and the picture that draw() states: record f has its TRACE floats at state + f * stride.  OSA_EINVAL
 * before any launch on the conditions of osa_render_episode and for a level outside 0 .. LEVELS; OSA_EUNSUPPORTED for
 * a description without draw(). */
int osa_custom_render_episode(int level, const float* state, long stride, int first, int count, int trail,
                              const uint8_t* hit, int camera, int width, int height, int supersample, uint8_t* rgb,
                              void* stream);

/* The runtime parameters of the description: *count = PARAMS (0 without the member); defaults (may be NULL): PARAMS
 * floats, room for 16; names (may be NULL): PARAM_NAMES with one space between two of them and a terminating 0, in at
 * most cap bytes -- OSA_EINVAL where they do not fit. */
int osa_custom_param_info(int* count, float* defaults, char* names, int cap);

/* The parameter-taking forms: the plain form's arguments, and in front of the stream `range` (the (2, P) ranges),
 * `par` and `ld_par` (rows of P floats at stride ld_par >= P).  OSA_EUNSUPPORTED in a library without PARAMS (as the
 * plain forms in a library with PARAMS), before any other check; OSA_EINVAL for a null range or par or ld_par < P.
 *   step     par is the (N, ld_par) matrix of the envs' current rows, read and (at a reset) rewritten
 *   eval     par receives row k of episode k: the (K, P) record of what every episode was played under
 *   collect  par receives the row lane k holds when the launch ends
 *   render   one row `par` of P floats (no ld_par): the parameters of the episode drawn, OsaDrawAt::par of every frame;
 *            OSA_EINVAL for a null par */
int osa_custom_env_step_params(unsigned long long seed, unsigned long long step, const unsigned long long* step_base,
                               int N, int obs_dim, int horizon, int level, float* state, int* steps,
                               const float* action, int ld_action, float* obs, int ld_obs, float* reward, float* cost,
                               uint8_t* terminated, uint8_t* truncated, float* final_obs, int ld_final, int reset_only,
                               const float* range, float* par, int ld_par, void* stream);
int osa_custom_eval_episodes_params(int level, int K, int obs_dim, int act_dim, int hidden, const float* params,
                                    const float* norm_mean, const float* norm_std, const long* norm_count,
                                    float norm_clip, const float* old_min, const float* old_max, float min_action,
                                    float max_action, unsigned long long seed, int horizon, float cost_p,
                                    int max_steps, int saute, float saute_budget, float saute_gamma,
                                    int early_terminated, double cost_limit, double cost_criteria, double* ep_ret,
                                    double* ep_cost, int* ep_len, float* trace, const float* range, float* par,
                                    int ld_par, void* stream);
int osa_custom_collect_episodes_params(int level, int K, int rows_per_lane, long total_rows, int obs_dim, int act_dim,
                                       int hidden, const float* params, const float* norm_mean, const float* norm_std,
                                       const long* norm_count, float norm_clip, const float* old_min,
                                       const float* old_max, float min_action, float max_action,
                                       unsigned long long seed, unsigned long long noise_seed, int horizon,
                                       float cost_p, float* obs, int ld_obs, float* action, int ld_act, float* reward,
                                       float* cost, float* next_obs, int ld_next, float* done, double* ep_ret_sum,
                                       double* ep_cost_sum, int* ep_count, const float* range, float* par, int ld_par,
                                       void* stream);
int osa_custom_render_episode_params(int level, const float* state, long stride, int first, int count, int trail,
                                     const uint8_t* hit, int camera, int width, int height, int supersample,
                                     uint8_t* rgb, const float* par, void* stream);

#ifdef __cplusplus
}
#endif
#endif
