/* daisyworld_hip.h — C ABI of libdaisyworld_hip.so, the MI355X (gfx950) implementation of the
 * RLDaisyWorld grid-update hot path.
 *
 * The reference (riveSunder/therldaisyworld) is pure Python/NumPy and has no FFI layer: the
 * "operator interface" of this path is the method surface of class RLDaisyWorld in
 * daisy/daisy_world_rl.py.  Each entry point below therefore cites the reference method
 * (file:line) whose work it performs.  The Python drop-in therldaisyworld_amd.RLDaisyWorld binds
 * these functions with ctypes (see INTEGRATION.md for the stub a reference maintainer would add).
 *
 * Conventions
 *   - plain C: opaque handle, plain pointers and sizes; no C++/torch types cross the boundary.
 *   - every function returns DW_OK (0) or a negative DW_E* code and never throws; the message of
 *     the last failure on the calling thread is returned by dw_last_error().
 *   - the caller owns every host buffer (C-contiguous); the library owns all device memory inside
 *     the handle and frees it in dw_destroy().
 *   - a handle is bound to one HIP device and one stream; it is not thread-safe, distinct handles
 *     may be used from distinct threads / processes (one process per GPU for ensemble shards).
 *   - dw_step*, dw_policy_* and dw_init_random are asynchronous on the handle's stream; every
 *     function that returns data to the host synchronises that stream first.
 *   - there is NO CPU fallback: on a machine without a usable HIP device dw_create() fails with
 *     DW_ENODEVICE.
 *
 * Layout
 *   grids are row-major [world][row][col]; "row" is the reference's axis -2 (which its code calls
 *   x) and "col" its axis -1 (y).  Device state is two planar BINARY16 arrays per buffer (light,
 *   dark) holding the cover in PER-MILLE units (1000 * cover: exactly the integers 0..1000 once a
 *   step has run, because the reference quantises to 3 decimals, daisy_world_rl.py:452 - and binary16
 *   holds every integer up to 2048 exactly, so the format is lossless: 2 bytes per value, 8 bytes of
 *   HBM traffic per cell-update), kept ping-pong so that the pre-step state stays available for
 *   observations / materialisation.  An UN-quantised state (the reference's initial grid is not
 *   rounded, :285-324) stays in its upload format - float64, or float32 per-mille - until the first
 *   step has consumed it.
 *
 * Numerics of the default mode (DW_PRECISION_EXACT): the light / dark planes after any step, and
 * everything derived from quantised values (observations, rewards, done flags, lifespans, the rounded
 * temperature channels), are bit-identical to the reference's float64 NumPy path.  Two caveats, stated
 * here so that "bit-exact" is not read as a proof: (i) the reference convolves by FFT, this library by
 * the mathematically identical 9-tap stencil, and the float64 repair path forms T_x^4 directly instead
 * of through the chain of fourth roots - both differ from the reference by a few 1e-16 relative BEFORE
 * rounding, the size of the reference's own FFT noise; a cell whose float64 pre-rounding value lies
 * that close to a rounding tie could round differently (never observed: 2e10 cell-updates soaked
 * against the oracle on the round-3 kernels alone, 0 mismatches); (ii) un-quantised outputs - reset() observations, env.grid after
 * reset(), the temp / beta / growth caches - agree with the reference to ~1e-13 relative, not bit for bit.
 */
#ifndef DAISYWORLD_HIP_H
#define DAISYWORLD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DW_ABI_VERSION 6

/* ---- error codes ---------------------------------------------------------------------------- */
enum {
    DW_OK = 0,
    DW_EINVAL = -1,     /* bad argument (null pointer, shape mismatch, unsupported size) */
    DW_ENODEVICE = -2,  /* no usable HIP device / wrong architecture */
    DW_ENOMEM = -3,     /* device or host allocation failed */
    DW_EHIP = -4,       /* a HIP runtime call failed (message has the HIP error string) */
    DW_ESTATE = -5      /* call not valid in the handle's current state (e.g. step before upload) */
};

/* ---- arithmetic modes ----------------------------------------------------------------------- */
enum {
    /* float32 arithmetic with a float64 re-evaluation of every cell whose pre-rounding value lies
     * within a proven error bound of a rounding tie: results are bit-identical to float64
     * evaluation of the reference formulas (the default). */
    DW_PRECISION_EXACT = 0,
    /* float32 arithmetic only: every cell within one quantum (1e-3) of the float64 result and
     * >= 99.98 % of the cell values identical after one step from the same state (measured >= 99.994 % on
     * developed states over the whole luminosity ramp, profiles/r02_fast_tolerance.json); ensemble means
     * of a trajectory within 3e-4.  A single small world's trajectory diverges cell-wise (one flipped tie
     * is amplified by the dynamics): that is what the exact mode is for. */
    DW_PRECISION_FAST = 1,
    /* float64 arithmetic for every cell (slow; the in-library reference the other two are tested
     * against).  (The exact mode's first step from an un-quantised initial state is float32 with an error bound
     * for non-integer inputs, float64 only for the cells that bound cannot decide: the same results.) */
    DW_PRECISION_F64 = 2
};

/* which of the two retained states a download refers to */
enum { DW_STATE_CURRENT = 0, DW_STATE_PREVIOUS = 1 };

/* scripted policy modes for dw_policy_greedy (ref: daisy/agents/greedy.py:14-36) */
enum { DW_POLICY_ARGMAX = 0, DW_POLICY_ARGMIN = 1 };

typedef struct dw_handle dw_handle;

/* Construction-time shape + the physics constants of RLDaisyWorld.__init__
 * (ref: daisy_world_rl.py:18-79).  Shapes are fixed for the life of the handle; the constants can
 * be changed later with dw_set_params (the reference lets callers assign attributes and then call
 * reset(), e.g. notebooks/greedy_longevity_abatement.ipynb cell 2:3-8). */
typedef struct dw_params {
    int32_t abi_version;      /* must be DW_ABI_VERSION */
    int32_t batch;            /* B: worlds in this handle (ref batch_size, :20).  No cap of its own: every call takes
                                 ensembles of more than 65 535 worlds (the launches that spread worlds over a grid
                                 dimension go in slices of that many); the limits are H*W <= 2^31-1 cells per world,
                                 B*H*W < 9e18 cells and the device's memory */
    int32_t height;           /* H = grid_dimension (:29) */
    int32_t width;            /* W = grid_dimension; H != W is allowed (ft_convolve accepts it) */
    int32_t n_agents;         /* N agents per world (:79); 0 allowed */
    int32_t device;           /* HIP device ordinal */
    int32_t precision;        /* DW_PRECISION_* */
    int32_t obs_mask;         /* 9-bit row-major 3x3 neighbourhood mask applied to observations
                                 (bit 4 = centre); von Neumann = 0x0BA, Moore = 0x1FF
                                 (ref: nn/functional.py:51-103, daisy_world_rl.py:261).  Any 9-bit value
                                 is admitted, 0 included, and may be changed on a live handle with
                                 dw_set_params: a greedy candidate it hides counts as 0.0, a corner it shows
                                 reaches the MLP policies (tested in every form: tests/test_gpu_obs_masks.py) */
    int32_t collision_mode;   /* 0 or 1 (ref :44, :220-242) */
    int32_t reserved0;
    int64_t world_offset;     /* global id of world 0 of this shard; keys the device RNG so that an
                                 ensemble sharded over GPUs draws the same worlds as a single run */
    double p, g, S, sigma, gamma, q, q2, dt;                         /* ref :32-52; g < 0 (a growth curve that opens
                                                                        upwards) only with DW_PRECISION_F64: the float32
                                                                        modes return DW_EINVAL for it */
    double albedo_bare, albedo_light, albedo_dark, temp_optimal;     /* ref :65-69 */
    double agent_gamma, food_chain_penalty;                          /* ref :55, :70 */
    double initial_al, initial_ad, light_proportion, dark_proportion;/* ref :73-77 */
} dw_params;

/* Per-world reductions fused into every step: the callers' lifespan test
 * `grid[:,1:3].max((1,2,3)) <= 0.005` (notebook greedy_longevity_abatement cell 2:48), the no-agent
 * reward `grid[:,1:3].sum((-2,-1)) > 0` (ref :489) and the population means.  All integers, in
 * per-mille units, hence exact and order-independent. */
typedef struct dw_world_stats {
    uint32_t max_k;        /* max over light and dark cells of 1000*cover */
    uint32_t reserved;     /* library-internal (a diagnostic count behind dw_last_fixup_count); do not interpret */
    uint64_t sum_light_k;  /* sum over cells of 1000*light */
    uint64_t sum_dark_k;   /* sum over cells of 1000*dark  */
} dw_world_stats;

/* ---- life cycle ----------------------------------------------------------------------------- */

/* Fill *p with the reference's default constants for the given shape (ref :18-79). */
int dw_default_params(dw_params* p, int32_t batch, int32_t height, int32_t width, int32_t n_agents);

/* Create a handle (allocates device state).  ref: RLDaisyWorld.__init__ :15-83 (without the RNG
 * draws, which stay on the host in the shim for same-seed parity, or use dw_init_random). */
int dw_create(const dw_params* p, dw_handle** out);
int dw_destroy(dw_handle* h);

/* Replace the physics constants (shape / device fields must match the handle's). */
int dw_set_params(dw_handle* h, const dw_params* p);
int dw_get_params(const dw_handle* h, dw_params* out);

const char* dw_last_error(void);
int dw_abi_version(void);

/* Page-locked host memory (hipHostMalloc) for buffers the library fills or reads: a download into it runs at the full
 * host-link rate, without the driver's staging copies (a pageable 4 MB reward block of dw_run_episode_mlp: 0.2 ms
 * instead of 0.5-2 ms, box dependent).  No reference counterpart; needs a gfx950 device (DW_ENODEVICE otherwise). */
int dw_pinned_alloc(size_t bytes, void** out);
int dw_pinned_free(void* p);
/* Hash of the sources + compiler flags this library was built from (16 hex digits; "unknown" for a build
 * that did not go through therldaisyworld_amd/build.py).  build.py rebuilds when it differs from the
 * sources in the tree, so a stale binary cannot run under newer host code. */
const char* dw_build_id(void);

/* ---- state in / out ------------------------------------------------------------------------- */

/* Upload an initial cover state, cover fractions in natural units [B][H][W] float64; the state is
 * treated as NOT quantised (ref initialize_grid :285-324 does not round): it is kept as uploaded, and the
 * next step reads these exact values (exact mode: float32 with a bound for non-integer inputs, the undecided
 * cells in float64 from the originals - bit-identical to a float64 evaluation).  Resets the retained
 * "previous" state. */
int dw_upload_state_f64(dw_handle* h, const double* light, const double* dark);

/* Same from float32 natural-unit planes.  quantised != 0 asserts every value is k/1000 (it is rounded to the
 * per-mille integer and goes straight into the binary16 planes); 0: the state is un-quantised, kept as float32
 * per-mille until the first step. */
int dw_upload_state_f32(dw_handle* h, const float* light, const float* dark, int quantised);

/* Agent positions [B][N][2] (row, col) and energy stores [B][N] (ref initialize_agents :173-179). */
int dw_upload_agents(dw_handle* h, const int32_t* indices, const double* states);
int dw_download_agents(dw_handle* h, int32_t* indices, double* states);

/* Synthetic initial state generated on the device with a counter-based RNG (Philox4x32-10 keyed by
 * seed, global world id and cell), same distribution as ref initialize_grid :287-302 and
 * initialize_agents :175-179: cover = [U1 < proportion] * initial_a * U2 per species, agents at
 * uniform cells with state 1.  Used for the large synthetic configurations. */
int dw_init_random(dw_handle* h, uint64_t seed);

/* The same draw with every cover rounded to three decimals (what np.round(., 3) would make of it), written
 * straight into the binary16 planes: a QUANTISED synthetic state.  Needs no float32 staging (dw_init_random holds
 * the un-quantised state in 8 bytes per cell until the second step) and no float64 first step; for ensembles that
 * fill the device.  Same worlds as dw_init_random up to that rounding (same keys). */
int dw_init_random_quantised(dw_handle* h, uint64_t seed);

/* Download light/dark cover of the current or previous state in natural units, [B][H][W] float64
 * (either pointer may be NULL). */
int dw_download_planes(dw_handle* h, int which, double* light, double* dark);

/* Materialise the reference's 7-channel grid `self.grid` [B][7][H][W] float64 for the current
 * state: after a step = exactly ref forward() :445-459 (rounded covers and bare, rounded
 * temperatures of the pre-step state, agent states written into channel 4); after an upload = ref
 * initialize_grid :304-323 (un-rounded).  L_init is used only in the second case. */
int dw_download_grid(dw_handle* h, double L_init, double* grid7);

/* Side-effect caches of the last physics pass, each optional (NULL to skip):
 * temps [B][3][H][W] = temp, temp_light, temp_dark (un-rounded; ref :415-419),
 * betas [B][3][H][W] = beta, beta_l, beta_d (ref :345-347), growth [B][2][H][W] (ref :373),
 * temp_effective [B][H][W] (ref :404).  L is the luminosity of that pass: ONE value for all worlds (after
 * dw_step_n_trace_per_world the caller's L is used as it stands, for every world). */
int dw_download_caches(dw_handle* h, double L, double* temps, double* betas, double* growth,
                       double* temp_effective);

/* ---- the hot path --------------------------------------------------------------------------- */

/* One environment step with luminosity L (ref step :475-497 minus update_L, which stays on the
 * host as a float64 scalar recurrence, :463-473):
 *   1. if action != NULL: update_agents (ref :181-244) for the leading action_b x action_n block
 *      of agents, host int32 actions [action_b][action_n] (codes 0..8);
 *   2. grid = forward(grid) (ref :434-461) as one fused stencil + reaction kernel;
 *   3. per-world reductions (dw_world_stats).
 * Asynchronous. */
int dw_step(dw_handle* h, const int32_t* action, int32_t action_b, int32_t action_n, double L);

/* dw_step followed by dw_get_obs and dw_get_reward_done with a single synchronisation: what one call of the
 * reference's step() returns (ref :475-497: obs, reward, done), for latency-bound small batches.  obs /
 * reward / done may be NULL. */
int dw_env_step(dw_handle* h, const int32_t* action, int32_t action_b, int32_t action_n, double L,
                double* obs /* [B][N][7][3][3] */, double* reward /* [B][N] */, uint8_t* done /* [B][N] */);

/* Same, taking the actions from the handle's device action buffer (filled by dw_policy_greedy or
 * dw_upload_actions) — keeps an episode loop free of host round trips. */
int dw_step_device_actions(dw_handle* h, double L);
int dw_upload_actions(dw_handle* h, const int32_t* action /* [B][N] */);
int dw_download_actions(dw_handle* h, int32_t* action /* [B][N] */);

/* `nsteps` consecutive steps with the reference's luminosity recurrence L <- clamp(L + dL)
 * (ref :471-473) evaluated on the host in float64, *L_io updated.  use_device_actions: 0 = no
 * update_agents call at all (ref `action is None` with n_agents == 0), 1 = actions are taken from
 * the device action buffer every step (constant unless a policy refreshes it).
 * The result equals `nsteps` calls of dw_step bit for bit; how the steps are issued is the library's business
 * (on wide grids two steps share one launch: step-1 values live only in registers). */
int dw_step_n(dw_handle* h, int32_t nsteps, double* L_io, double dL, double min_L, double max_L,
              int use_device_actions);

/* The time series of an agent-free run (the notebook's population curves, ref daisy/notebook_helpers.py:50-54): nsteps
 * steps (as dw_step_n with use_device_actions = 0) with luminosity L_schedule[t] for step t.
 * trace[t*B + b] = what dw_reduce would report for world b after step t (max_k, sum_light_k, sum_dark_k; `reserved` is
 * unspecified).  State, retained previous state, dw_reduce and observations after the call are those of nsteps calls of
 * dw_step(h, NULL, 0, 0, L_schedule[t]), bit for bit.  The series is recorded on the device (on wide grids by the step-pair
 * kernels themselves, see dw_kernel_info: "trace: step pairs" / "trace: single steps") and downloaded once per 32 MiB of
 * records.  nsteps == 0 is a no-op.  Synchronises (it fills a host buffer). */
int dw_step_n_trace(dw_handle* h, int32_t nsteps, const double* L_schedule, dw_world_stats* trace /* [nsteps][B] */);

/* The same run with a luminosity per WORLD: world b takes step t at L_schedule[t*B + b] (the luminosity enters the map
 * through the local temperature, ref daisy_world_rl.py:405,408) - an ensemble that scans the forcing in one call:
 * equilibrium cover against luminosity, collapse points, the hysteresis between a rising and a falling branch.  nsteps
 * single steps with no agent update; `trace` may be NULL, otherwise it is filled exactly as dw_step_n_trace fills it.
 * Afterwards the planes of world b, the retained previous state, dw_reduce and dw_last_fixup_count (summed over the
 * worlds) are what nsteps calls dw_step(h1, NULL, 0, 0, L_schedule[t*B + b]) leave on a ONE-world handle that holds
 * world b - bit for bit, in all three precisions, from a quantised or an un-quantised state.  W >= 256 (a multiple of
 * 4) steps by wave-strip kernels that read each world's constants from a device table by scalar loads, every other
 * shape and the first step from an un-quantised state by the one-thread-per-cell kernel (dw_kernel_info says which).
 * DW_EINVAL: null handle or schedule, or a luminosity that is not finite or is negative (checked before anything is
 * launched: the state is untouched); DW_ESTATE: no state; DW_ENOMEM: the table of constants could not be allocated
 * (nothing is kept: a later call allocates again).
 * The handle has no single luminosity of the last step afterwards, so whatever derives temperature channels from it -
 * dw_download_grid, dw_get_obs, the observations of dw_run_episode* - returns DW_ESTATE ("per-world") until a
 * shared-L step (dw_step, dw_step_n, dw_env_step, ...) or an upload / dw_init_random has been made.  dw_download_planes,
 * dw_reduce, dw_device_planes and the snapshots work as ever; dw_download_caches takes its L argument, ONE luminosity
 * for all worlds. */
int dw_step_n_trace_per_world(dw_handle* h, int32_t nsteps, const double* L_schedule /* [nsteps][B] */,
                              dw_world_stats* trace /* [nsteps][B], may be NULL */);

/* Per-world statistics of the local temperature field - the reference's `self.temp` (ref daisy_world_rl.py:410,415; NOT
 * temp_light / temp_dark), in kelvin, over the H*W cells of each world: the curves its notebooks append after every
 * step (`env.temp.mean()`, notebooks/daisy_world_existential_risk_and_agency.ipynb cell 2 run_q2_sims; `temp.mean()` and
 * `temp.std()`, daisy/notebook_helpers.py:50-52).  `std` is the population standard deviation (np.std, ddof = 0).  Always
 * evaluated in float64, whatever the handle's precision, from the same per-cell values as the `temps` cache of
 * dw_download_caches: min and max are two of those doubles.  The reduction is deterministic (fixed order, no atomics;
 * world b reduces the same whatever the batch) and takes the moments about the temperature of the world's cell (0, 0):
 * a uniform world has std == 0.0 and min == max == mean exactly. */
typedef struct dw_temp_stats { double mean, std, min, max; } dw_temp_stats;   /* 32 bytes, kelvin */

/* The statistics of the field dw_download_caches(h, L, temps, ...) returns as temps[:,0], without moving it: the same
 * source state (after a step the retained previous state, before any step the uploaded one) and the same rule for the
 * luminosity (the handle's last shared luminosity once a shared-L step has run; the caller's L otherwise - ONE value for
 * all worlds - including after a per-world run).  After dw_step(h, NULL, 0, 0, L) it is what the reference's env.temp
 * holds after that step (ref :415).  Synchronises.  DW_EINVAL: null argument; DW_ESTATE: no state; DW_ENOMEM: the
 * reduction's buffers could not be allocated (nothing is kept). */
int dw_reduce_temperature(dw_handle* h, double L, dw_temp_stats* per_world /* [B] */);

/* The temperature series of an agent-free run (ref run_q2_sims, daisy/notebook_helpers.py:50-52): nsteps single steps
 * without agents, and temps[t*B + b] = the statistics of the temperature field step t computes - world b's state BEFORE
 * step t at that step's luminosity, which is what env.temp holds after the t-th env.step() (ref :415,437).
 * per_world == 0: L_schedule[nsteps], one luminosity per step as dw_step_n_trace; per_world != 0:
 * L_schedule[nsteps][B] as dw_step_n_trace_per_world, with its validation and error codes, and the handle is "per-world"
 * afterwards as after that call.  `trace`, when given, is filled exactly as those calls fill it.  Planes, retained
 * previous state, dw_reduce and dw_last_fixup_count afterwards are those of dw_step_n_trace / dw_step_n_trace_per_world
 * with the same schedule, bit for bit; the first step from an un-quantised state reads it in its own format.
 * The temperatures are reduced by a kernel of their own that reads each step's input planes in front of the step, so
 * the steps are taken one launch each, never in fused pairs: that is the price of the series.
 * Records stay on the device and are downloaded once per 32 MiB.  nsteps == 0 is a no-op.  Synchronises.
 * DW_EINVAL: null handle, schedule or temps (and, per world, a luminosity that is not finite or is negative: the state
 * is untouched); DW_ESTATE: no state; DW_ENOMEM: a buffer could not be allocated (nothing is kept). */
int dw_step_n_trace_temperature(dw_handle* h, int32_t nsteps, const double* L_schedule, int per_world,
                                dw_world_stats* trace /* [nsteps][B], may be NULL */,
                                dw_temp_stats* temps  /* [nsteps][B] */);

/* Spatial frames: the image panels of the reference's figure (daisy/notebook_helpers.py plot_grid / update_fig:
 * tensor_to_image(env.grid[:, :3]) and tensor_to_image(env.temp)) without moving the planes.  A frame holds, per tile of
 * tile_h x tile_w cells of each selected world, the exact integer sums of the light and dark per-mille cover and the
 * float64 mean of the local temperature (kelvin).  TH = H / tile_h, TW = W / tile_w tiles per world, row-major; at 1 x 1
 * tiles a frame is env.grid[:, 1], env.grid[:, 2] (times 1000) and env.temp themselves. */
typedef struct dw_tile_cover { uint32_t sum_light_k, sum_dark_k; } dw_tile_cover;   /* 8 bytes, per-mille integers */
typedef struct dw_frame_spec {
    int32_t tile_h, tile_w;        /* must divide H and W; tile_h * tile_w <= 1 048 576 (the sums fit 32 bits) */
    int32_t n_worlds;              /* S: number of selected worlds; 0 with worlds == NULL: all B, in order */
    const int32_t* worlds;         /* [S] distinct world indices in 0..B-1, any order */
} dw_frame_spec;

/* One frame of the handle's state, on demand (also the way to frames of a per-step loop WITH agents: one call after each
 * dw_step / dw_env_step).
 *   cover      the tile sums of the CURRENT state, which must be quantised: DW_ESTATE ("the current state is not quantised
 *              yet; take the first step with dw_step") before the first step after an un-quantised upload.
 *   temp_mean  the tile means of the field dw_reduce_temperature(h, L, .) reduces - the same source state (after a step the
 *              retained previous state, in its own format while that is the un-quantised upload), the same rule for L,
 *              DW_ESTATE in the same cases.  Every cell's temperature is the double dw_download_caches returns in
 *              temps[:, 0]: float64 in all three precisions.  The sum of a tile is taken in a fixed order that depends on
 *              (tile_h, tile_w) only - not on B, the selection or the entry point; no atomics: world b's bytes are the
 *              same alone and in any ensemble, and a 1 x 1 tile is the cell's double itself.
 * At least one of the two is required.  Only the selected worlds are evaluated.  Synchronises.
 * DW_EINVAL (checked before anything is launched or allocated): a null handle or spec, both outputs null, a tile that does
 * not divide the grid or has more than 2^20 cells, n_worlds < 0, n_worlds > 0 with null worlds, a world index out of range
 * or listed twice, a luminosity that is not finite or is negative; DW_ESTATE: no state (and the cases above);
 * DW_ENOMEM: the frame buffers could not be allocated (nothing is kept). */
int dw_reduce_tiles(dw_handle* h, double L, const dw_frame_spec* spec,
                    dw_tile_cover* cover /* [S][TH][TW], may be NULL */, double* temp_mean /* [S][TH][TW], may be NULL */);

/* dw_step_n_trace with frames: nsteps agent-free steps at L_schedule[t] (no agent update is made, with or without agents on
 * the handle), and a frame at every stride-th step: F = nsteps / stride frames, frame f belongs to step
 * t_f = (f + 1) * stride - 1.  Steps after the last whole stride are taken and recorded in `trace`, but have no frame.
 *   cover[f]      the tile sums of the state AFTER step t_f: the tiles of a world sum to trace[t_f]'s sums.
 *   temp_mean[f]  the tile means of the field step t_f COMPUTES - the state before it at L_schedule[t_f], the row convention
 *                 of dw_step_n_trace_temperature: what env.temp holds after t_f + 1 calls of env.step().  The bytes are
 *                 those dw_reduce_tiles returns for that state.
 * Planes, retained previous state, dw_reduce, dw_last_fixup_count and `trace` afterwards are those of dw_step_n_trace with
 * the same schedule, bit for bit, in all three precisions, from a quantised or an un-quantised state.  A frame step is a
 * single launch (its input and its output planes are in HBM around it); the steps between two frames pair where
 * dw_step_n_trace would pair a run of their number.  Frames wait on the device and are downloaded once per 32 MiB of frame
 * records (a larger frame on its own); there is no other host synchronisation between the steps.  A call without temp_mean
 * evaluates no float64 field.  nsteps == 0 is a no-op.  Synchronises.
 * DW_EINVAL (before anything is launched or allocated; the state is untouched): dw_reduce_tiles' cases, a null L_schedule,
 * stride < 1, nsteps < 0; DW_ESTATE: no state; DW_ENOMEM: a buffer could not be allocated (nothing is kept).
 * Out of scope: per-world luminosities or constants.  Frames of a run with agents: dw_run_episode_frames. */
int dw_step_n_frames(dw_handle* h, int32_t nsteps, const double* L_schedule /* [nsteps] */, const dw_frame_spec* spec,
                     int32_t stride, dw_tile_cover* cover /* [F][S][TH][TW], may be NULL */,
                     double* temp_mean /* [F][S][TH][TW], may be NULL */, dw_world_stats* trace /* [nsteps][B], may be NULL */);

/* Per-world physics constants: the members of dw_params a world of an ensemble call may have of its own (ref
 * daisy_world_rl.py:32-52, :65-69) - a sweep over q2, gamma, the albedos, temp_optimal or dt as ONE traced run instead of
 * one handle and one run per value (the reference's run_q2_sims runs its ramp three times with env.q2 = 0, q/64, q/8). */
typedef struct dw_world_params {
    double p, g, S, sigma, gamma, q, q2, dt, albedo_bare, albedo_light, albedo_dark, temp_optimal;
} dw_world_params;                                   /* 96 bytes */

/* The handle's own set (what every world of it steps with in every other call).  DW_EINVAL: null argument. */
int dw_world_params_of(const dw_handle* h, dw_world_params* out);

/* nsteps agent-free steps, world b with the constants worlds[b] (fixed for the whole call) and step t of it at the
 * luminosity L_schedule[t*B + b].  Afterwards the planes of world b, the retained previous state and dw_reduce are what
 * a ONE-world handle leaves that holds world b, carries those constants (dw_set_params) and takes nsteps calls of
 * dw_step(h1, NULL, 0, 0, L) - bit for bit, in all three precisions, from a quantised or an un-quantised state.
 * `trace` (may be NULL) is filled exactly as dw_step_n_trace_per_world fills it; `temps` (may be NULL) exactly as
 * dw_step_n_trace_temperature(per_world = 1) fills it, each world's field at its own constants.  dw_last_fixup_count is
 * the sum over the worlds of what that one-world handle reports after dw_step_n_trace (dw_step_n_trace_temperature when
 * `temps` is given) with the world's column.
 * Without `temps`, DW_PRECISION_FAST on un-packed wave-strip shapes other than W == 1024 takes the steps from a
 * quantised state in fused PAIRS (trace_pair_fast_pw: each strip reads its world's two coefficient sets from a device
 * table by scalar loads), with the pairing rule of dw_step_n_trace; a step without a partner, every step with `temps`,
 * the other precisions and every other shape take the single-step kernels of dw_step_n_trace_per_world
 * (dw_kernel_info: "per-world constants: step pairs" / "wave strips" / "generic").  The albedo-symmetric form of the exact kernels is used only when EVERY world's albedos are exactly
 * symmetric about the bare ground's; results do not depend on it.
 * Checked before anything is launched or allocated (the state is untouched) - DW_EINVAL: null h, worlds or L_schedule;
 * a luminosity that is not finite or is negative; a world whose set dw_set_params would refuse on this handle (g < 0
 * in the float32 precisions; the message names the world and the member).  DW_ESTATE: no state.  DW_ENOMEM: a buffer
 * could not be allocated (nothing is kept: a later call allocates again).  nsteps == 0 is a no-op.  Synchronises.
 * The handle's own dw_params is unchanged, and the handle is "per-world" afterwards as after
 * dw_step_n_trace_per_world: dw_download_grid, dw_get_obs and the observations of dw_run_episode* return DW_ESTATE
 * until a shared-L step, an upload or dw_init_random - and after THIS call so do dw_download_caches and
 * dw_reduce_temperature, which have no single constant set to evaluate the retained state with.  The snapshots save and
 * restore that mark. */
int dw_step_n_trace_ensemble(dw_handle* h, int32_t nsteps,
                             const dw_world_params* worlds /* [B] */,
                             const double* L_schedule      /* [nsteps][B] */,
                             dw_world_stats* trace         /* [nsteps][B], may be NULL */,
                             dw_temp_stats* temps          /* [nsteps][B], may be NULL */);

/* Measurement aid (bench.py): duration of the run of fused step-pair launches issued by the LAST
 * dw_step_n call, from HIP events recorded on the handle's stream immediately before the first and after the
 * last of them (synchronises).  fused_launches = 0 (and fused_ms = 0) if that call issued none.
 * plane_elem_bytes = sizeof of the plane element those launches read and write (2: binary16). */
int dw_last_step_n_timing(dw_handle* h, float* fused_ms, int32_t* fused_launches, int32_t* plane_elem_bytes);

/* update_agents alone (ref :181-244) and forward alone on caller data (ref :434-461).  With
 * collision_mode = 1 dw_update_agents stops before the final clip: the reference's collision pass
 * (:220-242) draws from the caller's legacy RNG once per multiply-occupied cell, so the caller applies
 * it to the downloaded agent states, clips and uploads them (the Python drop-in does), then steps
 * without actions; dw_step / dw_run_episode with actions refuse collision_mode = 1.  dw_forward_f64
 * is stateless w.r.t. the cover planes: host covers [B][H][W] float64 in, 7-channel grid out
 * (agent states of the handle are written into channel 4 as the reference does); the optional
 * cache outputs are those of dw_download_caches for that input. */
int dw_update_agents(dw_handle* h, const int32_t* action, int32_t action_b, int32_t action_n);
int dw_forward_f64(dw_handle* h, const double* light, const double* dark, double L, double* grid7,
                   double* temps, double* betas, double* growth, double* temp_effective);

/* One 3x3 toroidal convolution of a caller-supplied float64 plane [B][H][W] with the 9 row-major kernel weights -
 * exactly the operation of ft_convolve (ref daisy/nn/functional.py:12-49, a true convolution on the torus) that
 * calculate_albedo (ref :377-394) and calculate_daisy_density (ref :423-432) are built from.  The drop-in's module-level
 * therldaisyworld_amd.nn.functional.ft_convolve(grid, kernel) calls it (the calculate_* methods use dw_stage_f64, the step
 * kernels fuse their stencils).  Does not touch the handle's state. */
int dw_conv3x3_f64(dw_handle* h, const double* plane, const double kernel[9], double* out);

/* The stages of forward() as stand-alone float64 maps on caller data, evaluated on the device (the drop-in's
 * calculate_* methods; forward() and step() use the fused kernels, never these).  `in` / `out`: host arrays of
 * whole planes, [plane][B][H][W] float64; `L`: the luminosity of the pass (stage 3); `kernel`: the nine row-major
 * weights of the stage's 3x3 toroidal convolution (stages 1, 2; ft_convolve, ref daisy/nn/functional.py:12-49).
 *   DW_STAGE_ALBEDO       ref calculate_albedo :377-394         in  bare (ignored: recomputed as p - l - d, ref :381), light, dark
 *                                                                out local albedo, adjacent albedo, bare
 *   DW_STAGE_DENSITY      ref calculate_daisy_density :423-432  in  light, dark           out density_light, density_dark
 *   DW_STAGE_TEMPERATURE  ref calculate_temperature :396-421    in  local, adjacent albedo out temp_effective, temp, temp_light, temp_dark
 *   DW_STAGE_GROWTH_RATE  ref calculate_growth_rate :340-348    in  temp, temp_light, temp_dark out beta, beta_l, beta_d
 *   DW_STAGE_GROWTH       ref calculate_growth :350-375         in  beta_l, beta_d, density_light, density_dark out growth_light, growth_dark
 * Does not touch the handle's state. */
#define DW_STAGE_ALBEDO 1
#define DW_STAGE_DENSITY 2
#define DW_STAGE_TEMPERATURE 3
#define DW_STAGE_GROWTH_RATE 4
#define DW_STAGE_GROWTH 5
int dw_stage_f64(dw_handle* h, int stage, const double* in, double* out, double L, const double kernel[9]);

/* Observations (ref get_obs :246-263): [B][N][7][3][3] float64 for the handle's agents, taken from
 * the current grid exactly as dw_download_grid would materialise it, times the neighbourhood mask. */
int dw_get_obs(dw_handle* h, double L_init, double* obs);

/* reward [B][N] float64 and done [B][N] uint8 as ref step :486-492 (N > 0). */
int dw_get_reward_done(dw_handle* h, double* reward, uint8_t* done);

/* Per-world reductions of the current state (always up to date after a step). */
int dw_reduce(dw_handle* h, dw_world_stats* per_world /* [B] */);

/* Scripted policy on the device (ref Greedy.__call__ agents/greedy.py:14-36): fills the device
 * action buffer from the current observations.  mode: DW_POLICY_ARGMAX -> 4+argmax of light+dark
 * over the candidates (row,col-1),(row-1,col),(row+1,col),(row,col+1) (= flat 3x3 indices 3,1,7,5),
 * first maximum wins; DW_POLICY_ARGMIN -> 4+argmin.  The epsilon (uniformly random) branch is
 * drawn by the caller (so that the legacy NumPy stream stays on the host) and handed over with
 * dw_upload_actions. */
int dw_policy_greedy(dw_handle* h, int mode);

/* Mixed-policy ensembles (BASELINE configs[4]: policy chosen by agent index): agent_mode[N] per agent
 * index DW_POLICY_ARGMAX, DW_POLICY_ARGMIN, or DW_POLICY_TABLE = keep the action already in the device
 * action buffer (host-drawn random actions put there with dw_upload_actions). */
int dw_policy_per_agent(dw_handle* h, const int32_t* agent_mode);

/* Learned policy on the device (ref MLP.get_action, daisy/agents/mlp.py:97-116):
 * the 63 -> 16 -> 32 -> 9 ReLU network evaluated in float64 on the current observations of agents
 * [agent_begin, agent_end) of every world; argmax of the logits goes to the device action buffer.
 * params: host float64[1808], the three weight matrices raveled row-major in layer order (ref
 * get_parameters :118-125).  Two calls with the two halves of the agents reproduce the agent /
 * adversary split of sges.get_fitness (daisy/evo/sges.py:163-168). */
int dw_policy_mlp(dw_handle* h, const double* params, int32_t n_params, int32_t agent_begin, int32_t agent_end,
                  double L_init);

/* The same for a whole population at once: params is [n_members][1808] and world_member[B] names the
 * parameter set each world's agents use, so that an evolution strategy evaluates all its members as ONE
 * batched ensemble instead of one episode per member (the reference farms members out to MPI workers,
 * daisy/evo/sges.py:314-349). */
int dw_policy_mlp_population(dw_handle* h, const double* params, int32_t n_members, const int32_t* world_member,
                             int32_t agent_begin, int32_t agent_end, double L_init);

/* Device-resident fitness episode of an evolution strategy (ref SimpleGaussianES.get_fitness,
 * daisy/evo/sges.py:144-181, and the population loop :314-349): K consecutive steps in which agents
 * [0, split) of world b act with MLP parameter set member_a[b] and agents [split, N) with member_b[b]
 * (ref: `agent` drives the first half, `adversary` the second, :165-168).  Parameters and member maps go
 * to the device once; per step: observations (ref get_obs :246-263), MLP.get_action (agents/mlp.py:97-116),
 * update_agents, forward; the step's reward = state * (state > 0) and done = reward < 0.1 (ref :486-492)
 * come back as [K][B][N].  member_a / member_b may be NULL when n_members == 1.  L_init: luminosity of the
 * observations' temperature channels if no step has been taken yet.  Worlds of H*W <= 4096 cells run the chunk as
 * ONE launch with the worlds resident in LDS (csrc/dw_episode.hpp: episode_mlp) once the state and the retained
 * previous state are quantised - i.e. from the third step of an episode on; larger worlds and the first two
 * steps take one launch sequence per step.  Same results either way.
 * ABI 4: `params` may be NULL - the parameter sets of the last call on this handle that passed them stay on the device
 * and are used again (n_members must be the same): a fitness harness uploads a population once per generation, not
 * once per chunk.  `reward` / `done` in page-locked memory (dw_pinned_alloc) are filled without a staging copy. */
int dw_run_episode_mlp(dw_handle* h, int32_t nsteps, const double* L_schedule, const double* params /* [n_members][1808] */,
                       int32_t n_members, const int32_t* member_a /* [B] */, const int32_t* member_b /* [B] */,
                       int32_t split, double L_init, double* reward /* [K][B][N] */, uint8_t* done /* [K][B][N] */);

/* The bookkeeping of those fitness episodes on the device (additive, ABI 6): what the reference's loop keeps per step,
 * daisy/evo/sges.py:160-176 - whether every agent is done, one more step counted in done_at and total_steps for every
 * agent that is not, the mean reward of the first half of the agents added to the sum, and the loop left behind the step
 * at which all are done - per member of a population evaluated as one ensemble: member block m owns worlds [m * worlds_per_member,
 * (m + 1) * worlds_per_member), P = B / worlds_per_member blocks (worlds_per_member = B: the single pair of get_fitness).
 * The accumulators stay on the device: sum_reward[P] float64, done_at[B][N] int32 (total_steps is the same count),
 * running[P].  A chunk of K steps is accounted for t = 0 .. K-1 in order; where member m runs at the start of step t:
 * done_at[b][n] += !done[t][b][n] for its worlds, sum_reward[m] += the mean of reward[t][b][0..half) over its worlds, and
 * the member stops running if every done flag of its block is set at step t.  That mean is the reference's call on the
 * block bit for bit: the n = worlds_per_member * half values taken world-major and agent-minor, added in NumPy's pairwise
 * order (csrc/dw_fitness_order.hpp) and divided by n with a correctly rounded float64 division.
 * *executed = 1 + the first t after which no member runs, with *finished = 1; otherwise *executed = K, *finished = 0 (a
 * chunk accounted when no member runs: 1 and 1, and nothing changes).  Steps behind `executed` change nothing.
 *   dw_fitness_begin     zeroes sums and counters, every member running
 *   dw_fitness_account   accounts the host arrays reward / done [K][B][N] of a chunk (uploads them)
 *   dw_run_episode_mlp_fitness   dw_run_episode_mlp with reward = done = NULL - it leaves planes, agents, actions, the
 *                        resident parameter sets and dw_last_fixup_count exactly so - and then accounts the chunk where
 *                        the episode kernels left its rewards and flags (every form of the call); 8 bytes come down
 *   dw_fitness_download  the accumulators (any pointer may be NULL); synchronises
 * DW_EINVAL: worlds_per_member does not divide B, half outside 1..N, nsteps outside 1..4096, a null handle or array;
 * DW_ESTATE: account, run or download before dw_fitness_begin; each leaves the handle untouched.  The accumulators are
 * not part of the snapshots: a harness that replays the executed steps of a chunk does so with dw_run_episode_mlp. */
int dw_fitness_begin(dw_handle* h, int32_t worlds_per_member, int32_t half);
int dw_fitness_account(dw_handle* h, int32_t nsteps, const double* reward /* [K][B][N] */, const uint8_t* done /* [K][B][N] */,
                       int32_t* executed, int32_t* finished);
int dw_run_episode_mlp_fitness(dw_handle* h, int32_t nsteps, const double* L_schedule, const double* params /* [n_members][1808] */,
                               int32_t n_members, const int32_t* member_a /* [B] */, const int32_t* member_b /* [B] */,
                               int32_t split, double L_init, int32_t* executed, int32_t* finished);
int dw_fitness_download(dw_handle* h, double* sum_reward /* [P] */, int32_t* done_at /* [B][N] */, uint8_t* running /* [P] */);

/* Device-side snapshot of the handle's state (current planes, the retained previous state that
 * observations and caches are derived from, agents, per-world reductions) and its restoration: lets an episode harness run chunks of steps ahead (dw_run_episode) and, when the episode
 * turns out to have ended inside a chunk, replay exactly the steps the reference's loop
 * (notebooks/greedy_longevity_abatement.ipynb cell 2:28-57: stop as soon as every world is dead) would
 * have executed — without moving the state over PCIe.  Costs up to two extra copies of the two planes
 * in HBM, allocated at the first save. */
int dw_snapshot_save(dw_handle* h);               /* = slot 0 */
int dw_snapshot_restore(dw_handle* h);
/* Two slots (ABI 5): a harness that lets the device run chunk c + 1 while the host still accounts for chunk c
 * (therldaisyworld_amd/harness.py, the ES fitness episodes: ref daisy/evo/sges.py:144-181) saves the start of chunk c in
 * slot c % 2 - when chunk c turns out to end the episode, the state at its start is still there although chunk c + 1 has
 * saved its own.  A save is one kernel launch for all regions of the state. */
#define DW_SNAPSHOT_SLOTS 2
int dw_snapshot_save_slot(dw_handle* h, int32_t slot);
int dw_snapshot_restore_slot(dw_handle* h, int32_t slot);

/* Device-resident lifespan harness (ref notebooks/greedy_longevity_abatement.ipynb cell 2:28-57):
 * accumulate done_at[b] += (max_k > threshold_k) and agents_done_at[b][n] += !(done) after each
 * step, on the device.  dw_lifespan_reset zeroes them. */
int dw_lifespan_reset(dw_handle* h);
int dw_lifespan_accumulate(dw_handle* h, uint32_t threshold_k);
int dw_lifespan_download(dw_handle* h, int32_t* done_at /* [B] */, int32_t* agents_done_at /* [B][N] */,
                         int32_t* n_worlds_alive);

/* Device-resident episode loop: K consecutive environment steps — policy,
 * update_agents (ref :181-244), forward (ref :434-461), reductions — without a host round trip per
 * step.  Small worlds (H*W <= 4096) run in ONE launch with the worlds held in LDS (H*W <= 256 - the reference's own 8x8
 * and 16x16 worlds - one wave per world with no workgroup barrier in the step: csrc/dw_episode_wave.hpp); larger worlds run the
 * same K steps as back-to-back launches on the handle's stream (policy / table slice, update_agents, the
 * streaming step kernel, flags from its reductions) with one synchronisation at the end.  It is the body of the
 * reference's lifespan harness (notebooks/greedy_longevity_abatement.ipynb cell 2:28-57) and of
 * sges.get_fitness (daisy/evo/sges.py:144-181) for scripted policies.
 *   L_schedule[K]   luminosity of each step (the caller runs the ref update_L recurrence :463-473)
 *   policy_mode     DW_POLICY_ARGMAX / DW_POLICY_ARGMIN (ref Greedy, agents/greedy.py:18-30),
 *                   DW_POLICY_ZEROS (ref step(None): action 0), DW_POLICY_TABLE (all actions given)
 *   use_table[K]    per step: 1 = this step's actions come from `table` (Greedy's epsilon branch,
 *                   drawn by the caller from the legacy NumPy stream); may be NULL (all 0)
 *   table[K][B][N]  int8 codes: 0..8 an action, -1 / -2 the greedy / anti-greedy choice of that agent at
 *                   that step (mixed-policy ensembles, BASELINE configs[4]); may be NULL if never used
 *   world_alive[K][B], agent_ok[K][B][N]   per-step flags out: max cover > threshold_k/1000, and
 *                   reward >= 0.1 (what the harness adds to done_at / agents_done_at)
 * world_alive may be NULL: without per-step world reductions wide grids (and big ensembles of narrow
 * ones) run step PAIRS as one fused launch, with the agents' step in between recomputed around the
 * agents and patched into the result (csrc/dw_agents_fused.hpp) - same results, bit for bit.
 * Needs a quantised current state (take the first step of an episode with dw_step).
 * Afterwards the handle is exactly as after K calls of dw_step (previous state retained; the device action buffer
 * - dw_download_actions - holds the resolved action codes of the LAST step, whichever kernel applied them). */
enum { DW_POLICY_ZEROS = 2, DW_POLICY_TABLE = 3 };
int dw_run_episode(dw_handle* h, int32_t nsteps, const double* L_schedule, int policy_mode,
                   const uint8_t* use_table, const int8_t* table, uint32_t threshold_k, uint8_t* world_alive,
                   uint8_t* agent_ok);

/* dw_run_episode with a set of physics constants and a luminosity column per WORLD: the reference's lifespan table
 * (notebooks/greedy_longevity_abatement.ipynb: albedo settings x policies, each an ensemble run until every biosphere is
 * dead) or a lifespan-versus-q2 / gamma / temp_optimal scan as ONE device-resident run instead of one handle
 * configuration and one run per scenario.  World b steps with worlds[b] (fixed for the whole call; the members of
 * dw_params that dw_world_params does not carry - agent_gamma, food_chain_penalty, obs_mask, the initial-state fields -
 * stay the handle's and are shared) and takes step t at L_schedule[t*B + b]; policy_mode, use_table, table, threshold_k
 * and the flags are dw_run_episode's (the per-world policy mix is the table's codes -1 / -2).
 * Contract: take a ONE-world handle that holds world b and its agents, carries worlds[b] (dw_set_params) and is given
 * column b of the schedule and slice [:, b] of the table.  Whatever dw_run_episode leaves on it - the planes, the
 * retained previous state, the agents, dw_reduce, the device action buffer, its world_alive / agent_ok columns - this
 * call leaves for world b, bit for bit, in DW_PRECISION_EXACT and DW_PRECISION_FAST; dw_last_fixup_count is the sum over
 * the worlds.
 * H*W <= 256 with at most 64 agents: one launch, one wave per world (episode_wave_pw, csrc/dw_episode_wave_pw.hpp: a wave
 * stages its own world's float32 rows of a 64-step segment in LDS and takes the float64 repair set from its world's
 * entry of a table); the rows - 136 bytes per step and world, all derived on the host in float64 by the functions that
 * serve dw_set_params - go up in one copy from a page-locked image.  Every other shape, DW_NO_EPISODE_WAVE and
 * DW_NO_EPISODE_KERNEL: launches per step from existing kernels (policy kernel or table slice, update_agents, the
 * per-world single step of dw_step_n_trace_ensemble, flags), one synchronisation at the end; no fused pairs, no LDS
 * workgroup kernel (dw_kernel_info: "; ensemble episode: one wave per world" / "launches per step").
 * Checked before anything is launched or allocated (the state is untouched): the rules of dw_run_episode (DW_ESTATE: no
 * state, no agents, an un-quantised current state; DW_EINVAL: DW_PRECISION_F64, collision_mode 1, nsteps outside 1..4096,
 * the table rules), of dw_step_n_trace_ensemble (DW_EINVAL: a luminosity that is not finite or is negative; a world whose
 * set dw_set_params would refuse - g < 0 - with a message that names the world and the member), null h, worlds or
 * L_schedule.  Synchronises.
 * Afterwards the handle is "per-world" in both senses, exactly as after dw_step_n_trace_ensemble: dw_get_obs,
 * dw_download_grid, dw_download_caches, dw_reduce_temperature and the observations of dw_run_episode* return DW_ESTATE
 * until a shared-L step, an upload or dw_init_random; the snapshots save and restore that mark. */
int dw_run_episode_ensemble(dw_handle* h, int32_t nsteps,
                            const dw_world_params* worlds /* [B] */,
                            const double* L_schedule      /* [nsteps][B] */,
                            int policy_mode, const uint8_t* use_table, const int8_t* table,
                            uint32_t threshold_k, uint8_t* world_alive, uint8_t* agent_ok);

/* dw_run_episode that also records, for every step and world, what dw_reduce would report after that step: the daisy
 * populations of an ensemble with grazing agents in it as ONE device-resident run - the curves of the reference's
 * animations with an agent (daisy/notebook_helpers.py:218-223 `update_fig_agent`, notebooks/rl_daisy_world.ipynb cells
 * 12-16, notebooks/greedy_longevity_abatement.ipynb cells 10-15: env.grid[:,1].mean() and env.grid[:,2].mean() appended
 * after every env.step(action)) - instead of one dw_step + dw_reduce round trip per step.
 * Contract: everything dw_run_episode leaves on the handle and in world_alive / agent_ok for the same arguments - the
 * planes, the retained previous state, the agents, dw_reduce, the device action buffer, dw_last_fixup_count, the flags -
 * this call leaves too, bit for bit, in DW_PRECISION_EXACT and DW_PRECISION_FAST (n_agents == 0 allowed).
 *   trace[t*B + b]  {max_k, sum_light_k, sum_dark_k} of world b after step t: the record dw_reduce returns after t + 1
 *                   single-step calls, written with reserved = 0.  Hence world_alive[t][b] == (trace[t*B+b].max_k >
 *                   threshold_k), and the last row equals dw_reduce after the call.  Required.
 * H*W <= 256 with at most 64 agents: one launch, one wave per world (episode_wave_stats_pw,
 * csrc/dw_episode_wave_stats_pw.hpp: the forward pass returns each lane's sums and maximum, combined across the wave with
 * DPP operations per step; the records of a 64-step segment wait in LDS and are written next to the segment's flags).
 * Every other shape, DW_NO_EPISODE_WAVE and DW_NO_EPISODE_KERNEL: launches per step from existing kernels (policy kernel
 * or table slice, update_agents, the step kernel, flags) plus one that copies the step's reductions into the trace - no
 * fused step pairs (the step-1 sums of a pair would have to include the patch kernel's corrections) and no LDS workgroup
 * kernel: the price of the records there (dw_kernel_info: "; episode trace: one wave per world" / "launches per step").
 * Flags and records come down through the staging buffer's page-locked image in one copy.
 * Checked before anything is launched or allocated (the state is untouched): the rules of dw_run_episode (DW_ESTATE: no
 * state, no agents, an un-quantised current state; DW_EINVAL: DW_PRECISION_F64, collision_mode 1, nsteps outside 1..4096,
 * the table rules), and DW_EINVAL for a null trace.  Synchronises. */
int dw_run_episode_trace(dw_handle* h, int32_t nsteps, const double* L_schedule, int policy_mode,
                         const uint8_t* use_table, const int8_t* table, uint32_t threshold_k,
                         uint8_t* world_alive /* [K][B], may be NULL */, uint8_t* agent_ok /* [K][B][N], may be NULL */,
                         dw_world_stats* trace /* [K][B], required */);

/* dw_run_episode_trace that also records, for every step and world, the statistics of the local temperature field that
 * step computes: the curves temp.mean() and temp.std() which the reference's animation with an agent appends after every
 * env.step(action) (daisy/notebook_helpers.py:210-223 `update_fig_agent`) - whether grazers break the biosphere's
 * temperature regulation - as ONE device-resident run, instead of one dw_step + dw_reduce_temperature round trip per step.
 * Contract: everything dw_run_episode_trace leaves on the handle and in world_alive / agent_ok / trace for the same
 * arguments - the planes, the retained previous state, the agents, dw_reduce, the device action buffer,
 * dw_last_fixup_count, the flags, the records - this call leaves too, bit for bit, in DW_PRECISION_EXACT and
 * DW_PRECISION_FAST (n_agents == 0 allowed).  `trace` may be NULL here.
 *   temps[t*B + b]  the dw_temp_stats of the field `self.temp` (ref daisy_world_rl.py:410,415) of world b in step t: taken
 *                   from the state AFTER step t's update_agents (grazed cells zeroed) and BEFORE its growth, at
 *                   L_schedule[t] - what env.temp holds after the t-th env.step(action).  Required.
 * Always float64, whatever the handle's precision: every cell's temperature is the float64 evaluation of the reference's
 * staging, and the reduction is the deterministic one of dw_reduce_temperature (moments about the temperature of the
 * world's cell (0, 0), the same association order).  Hence temps[K-1] equals dw_reduce_temperature(h, L_schedule[K-1], .)
 * after the call bit for bit, both forms below return identical bytes, and a world without cover has std == 0.0 and
 * min == max == mean.
 * The forms are dw_run_episode_trace's.  H*W <= 256 with at most 64 agents: one launch, one wave per world
 * (episode_wave_temp_pw, csrc/dw_episode_wave_temp_pw.hpp: each lane evaluates the temperature of its cells from the 3x3
 * neighbourhoods the forward pass loads; the wave reduces them in the order of the on-demand reduction; lane 0 stores the
 * step's 32-byte row).  Every other shape, DW_NO_EPISODE_WAVE and DW_NO_EPISODE_KERNEL: launches per step, with the
 * on-demand reduction's kernels between a step's update_agents and its step kernel (dw_kernel_info: "; episode
 * temperature: one wave per world" / "launches per step").  Flags, records and temperature rows come down in one copy.
 * Checked before anything is launched or allocated (the state is untouched): the rules of dw_run_episode_trace, and
 * DW_EINVAL for a null temps.  Synchronises. */
int dw_run_episode_trace_temperature(dw_handle* h, int32_t nsteps, const double* L_schedule, int policy_mode,
                                     const uint8_t* use_table, const int8_t* table, uint32_t threshold_k,
                                     uint8_t* world_alive /* [K][B], may be NULL */, uint8_t* agent_ok /* [K][B][N], may be NULL */,
                                     dw_world_stats* trace /* [K][B], may be NULL */, dw_temp_stats* temps /* [K][B], required */);

/* dw_run_episode_ensemble that also records, for every step and world, what dw_reduce would report after that step and
 * the statistics of the temperature field that step computes: the population and temperature curves of every scenario
 * of the reference's README - greedy, anti-greedy, random and no agents under light-and-dark and under neutral albedos,
 * compared side by side (daisy/notebook_helpers.py:210-223 `update_fig_agent` after every env.step(action)) - as ONE
 * device-resident run instead of one handle, one dw_set_params and one traced run per scenario.
 * Contract: everything dw_run_episode_ensemble leaves on the handle and in world_alive / agent_ok for the same
 * arguments - the planes, the retained previous state, the agents, dw_reduce, the device action buffer, the sum in
 * dw_last_fixup_count, the flags, the "per-world" marks (saved and restored by the snapshots), DW_POLICY_ZEROS winning
 * over use_table - this call leaves too, bit for bit, in DW_PRECISION_EXACT and DW_PRECISION_FAST (n_agents == 0 allowed).
 *   trace[t*B + b]  the record dw_run_episode_trace writes for step t on a ONE-world handle that holds world b and its
 *                   agents, carries worlds[b] (dw_set_params) and is given column b of the schedule and slice [:, b] of
 *                   the table; reserved = 0.  Hence world_alive[t][b] == (trace[t*B+b].max_k > threshold_k), and the last
 *                   row equals dw_reduce after the call.
 *   temps[t*B + b]  the row dw_run_episode_trace_temperature writes on that one-world handle: the field `self.temp` of
 *                   world b in step t, after the step's grazing and before its growth, at worlds[b] and
 *                   L_schedule[t*B + b].  float64 in both precisions, reduced in the order of dw_reduce_temperature: both
 *                   forms below return the same bytes, and a world without cover has std == 0.0 and min == max == mean.
 * At least one of trace and temps is required (flags only: dw_run_episode_ensemble); a call without temps evaluates no
 * float64 field.
 * The forms are dw_run_episode_ensemble's.  H*W <= 256 with at most 64 agents: one wave per world
 * (episode_wave_ens_trace_pw, csrc/dw_episode_wave_ens_trace_pw.hpp: episode_wave_pw's per-world rows in LDS with
 * episode_wave_temp_pw's records; a world's float64 set is loaded once per launch, wave-uniformly, and only its L changes
 * per step); a call whose rows pass 32 MiB takes several launches, each writing its flags and records from its first step's
 * row on.  Every other shape, DW_NO_EPISODE_WAVE and DW_NO_EPISODE_KERNEL: launches per step, with the on-demand
 * reduction's kernels at each world's float64 row of the step between update_agents and the step kernel (dw_kernel_info:
 * "; ensemble trace: one wave per world" / "launches per step").  Flags and records come down through the page-locked
 * image in one copy while the staging buffer is at most 64 MiB; beyond (4096 steps of 1000 worlds: 229 MB) the image
 * holds the inputs only and each output is copied straight into the caller's array.
 * Checked before anything is launched or allocated (the state is untouched): the rules of dw_run_episode_ensemble, and
 * DW_EINVAL when trace and temps are both null.  Synchronises.  Afterwards the handle is "per-world" as after
 * dw_run_episode_ensemble. */
int dw_run_episode_ensemble_trace(dw_handle* h, int32_t nsteps,
                                  const dw_world_params* worlds /* [B] */,
                                  const double* L_schedule      /* [nsteps][B] */,
                                  int policy_mode, const uint8_t* use_table, const int8_t* table,
                                  uint32_t threshold_k,
                                  uint8_t* world_alive /* [K][B], may be NULL */,
                                  uint8_t* agent_ok    /* [K][B][N], may be NULL */,
                                  dw_world_stats* trace /* [K][B], may be NULL */,
                                  dw_temp_stats* temps  /* [K][B], may be NULL */);

/* dw_run_episode_mlp that also records, for every step and world, what dw_reduce would report after that step and, on
 * demand, the statistics of the temperature field that step computes: the curves of the reference's trained-agent demo
 * (daisy/notebook_helpers.py:210-223 `update_fig_agent`, the existential-risk notebook's MLP cells: env.grid[:,1].mean(),
 * env.grid[:,2].mean(), temp.mean() and temp.std() appended after every env.step(action) while a trained MLP,
 * agents/mlp.py:97-116, grazes) without one host round trip per step.
 * Contract: everything dw_run_episode_mlp leaves for the same arguments - reward, done, the planes, the retained previous
 * state, the agents, dw_reduce, the device action buffer, dw_last_fixup_count, the parameter sets kept on the device for
 * a later params == NULL, the handle's shared-L marks - this call leaves too, bit for bit, in DW_PRECISION_EXACT and
 * DW_PRECISION_FAST.
 *   trace[t*B + b]  {max_k, sum_light_k, sum_dark_k} of world b after step t: the record dw_reduce returns after t + 1
 *                   single steps, reserved = 0.  The last row equals dw_reduce after the call.
 *   temps[t*B + b]  the dw_temp_stats of the field `self.temp` (ref daisy_world_rl.py:410,415) of world b in step t: after
 *                   that step's update_agents and before its growth, at L_schedule[t].  float64 in both precisions,
 *                   reduced in dw_reduce_temperature's order: the last row equals dw_reduce_temperature(h,
 *                   L_schedule[K-1], .) after the call, both forms below return the same bytes, and a world without cover
 *                   has std == 0.0 and min == max == mean.
 * At least one of trace and temps is required (rewards only: dw_run_episode_mlp); a call without temps evaluates no
 * float64 temperature field.
 * The forms (dw_kernel_info: "; mlp trace: one wave per world" / "launches per step").  H*W <= 256 with at most 4 agents,
 * once the current and the retained previous state are quantised: one wave per world (episode_mlp_wave_trace_pw,
 * csrc/dw_episode_mlp_wave_trace_pw.hpp: episode_mlp_wave's step with episode_wave_stats_pw's and episode_wave_temp_pw's
 * records).  Every other case - the workgroup shapes, larger worlds, DW_NO_EPISODE_WAVE, DW_NO_EPISODE_KERNEL, the first
 * steps of an episode - launches per step: observe, policy_mlp, grazing, with temps the on-demand temperature reduction
 * (on an un-quantised state in its own format), the step kernel, the record row.  There is no LDS workgroup kernel with
 * records: the price dw_run_episode_trace states.  A call that starts per step and continues in the wave kernel writes one
 * continuous set of rows.
 * Checked before anything is launched or allocated (the state is untouched): the rules of dw_run_episode_mlp, and
 * DW_EINVAL when trace and temps are both null.  DW_ENOMEM keeps nothing.  Synchronises. */
int dw_run_episode_mlp_trace(dw_handle* h, int32_t nsteps, const double* L_schedule, const double* params /* [n_members][1808] */,
                             int32_t n_members, const int32_t* member_a /* [B] */, const int32_t* member_b /* [B] */,
                             int32_t split, double L_init, double* reward /* [K][B][N], may be NULL */,
                             uint8_t* done /* [K][B][N], may be NULL */, dw_world_stats* trace /* [K][B], may be NULL */,
                             dw_temp_stats* temps /* [K][B], may be NULL */);

/* dw_run_episode_mlp_trace (cover records only) with a number of agents PER WORLD: the agent-count scans of the reference's
 * title notebook (notebooks/daisy_world_existential_risk_and_agency.ipynb, cells fd8ad489 .. 227e4895: n_agents over 1, 31,
 * 61, .. 271 on the 16x16 world, 10 worlds per count, under the trained MLP and the scripted policies) as ONE device-resident
 * run instead of one handle, one reset and one run per count.  In world b only agents [0, n_active[b]) exist.
 * An absent agent is not a dead one: the reference's forward stamps the state of every agent, dead or alive, into channel 4
 * at its cell (daisy_world_rl.py:454-459) and the MLP reads that channel, so the stamps of absent agents are not there.
 * Contract for world b, k = n_active[b]: take a one-world handle with n_agents = k that holds world b's planes (current and
 * retained previous state) and its first k agents, same precision and parameters, and step it K times with
 * dw_policy_mlp_population for [0, min(split, k)) with member_a[b] and for [min(split, k), k) with member_b[b], then
 * dw_step_device_actions, dw_get_reward_done, dw_reduce (k = 0: an agent-free handle, dw_step / dw_reduce).  This call
 * leaves for world b exactly what that handle holds, bit for bit, in DW_PRECISION_EXACT and DW_PRECISION_FAST: the planes,
 * the previous planes, dw_reduce, positions and states of agents < k, their entries of the action buffer, and reward /
 * done [:, b, :k]; trace[t*B + b] is that handle's dw_reduce after step t, reserved = 0.  dw_last_fixup_count is the sum
 * over the worlds of what those handles report.
 * Absent agents (n >= k): the state is set to 0.0 and stays 0.0, the position is left as uploaded, reward is 0 and done is 1
 * at every step, the action code is 0; they are neither observed nor stamped into channel 4.
 * The counts are an argument of THIS CALL, not a property of the handle: afterwards the handle has N agents of which those
 * have state 0, and a count-unaware call such as dw_get_obs sees them as dead agents (stamps included).
 * The forms (dw_kernel_info: "; mlp counts: workgroup (LDS)" / "launches per step", csrc/dw_counts_plan.hpp).  H*W <= 4096
 * where the LDS fits, once the current and the retained previous state are quantised: episode_mlp_counts_pw
 * (csrc/dw_episode_mlp_counts_pw.hpp), worlds in LDS with ~20 bytes per agent and 16 KiB of static LDS per workgroup for the
 * observation / activation blocks of its sixteen 16-lane groups.  Every other shape, the first steps of an episode and
 * DW_NO_EPISODE_KERNEL: launches per step (observe_counts_pw, policy_mlp, grazing, the step kernel, the record row).  Both
 * forms leave the same bytes.
 * Checked before anything is launched, allocated or uploaded (state and resident parameter sets untouched): the rules of
 * dw_run_episode_mlp; DW_EINVAL for a null n_active, for a count outside 0..N (the message names the world), for
 * collision_mode 1 and DW_PRECISION_F64.  All counts 0 is an agent-free run.  Synchronises. */
int dw_run_episode_mlp_counts(dw_handle* h, int32_t nsteps, const double* L_schedule, const double* params /* [n_members][1808] or NULL */,
                              int32_t n_members, const int32_t* member_a /* [B] */, const int32_t* member_b /* [B] */,
                              int32_t split, const int32_t* n_active /* [B], each in 0..N */, double L_init,
                              double* reward /* [K][B][N], may be NULL */, uint8_t* done /* [K][B][N], may be NULL */,
                              dw_world_stats* trace /* [K][B], may be NULL */);

/* dw_run_episode_trace_temperature with frames: the pictures of the reference's animation with an agent in it
 * (daisy/notebook_helpers.py:180-258 `update_fig_agent` redraws env.grid[:, :3], env.temp and the agent channel
 * env.grid[:, 4] after every env.step(action)) from ONE device-resident run, instead of one dw_run_episode of one step, one
 * dw_reduce_tiles and one dw_download_agents per step.  F = nsteps / stride frames; frame f belongs to step
 * t_f = (f + 1) * stride - 1, the rule of dw_step_n_frames; steps after the last whole stride are taken and recorded but
 * have no frame.  `spec` is dw_step_n_frames'.
 * Contract for the handle and the records: for the same arguments this call leaves what dw_run_episode_trace_temperature
 * leaves (without trace and temps: what dw_run_episode leaves) - the planes, the retained previous state, the agents,
 * dw_reduce, the device action buffer, dw_last_fixup_count, the flags, the records, the temperature rows - bit for bit, in
 * DW_PRECISION_EXACT and DW_PRECISION_FAST, n_agents == 0 allowed.
 * Contract for a frame: let "the state after t_f + 1 steps" be the handle after the first t_f + 1 steps of the call, taken
 * one dw_run_episode step at a time.
 *   cover[f]         byte for byte what dw_reduce_tiles(h, ., spec, cover, NULL) returns on that state: the tiles of
 *                    env.grid[:, 1] and env.grid[:, 2] after the step.
 *   temp_mean[f]     byte for byte what dw_reduce_tiles(h, ., spec, NULL, temp_mean) returns on that state: the field step
 *                    t_f computes from the grazed state at L_schedule[t_f] (env.temp after the step), in the same fixed
 *                    summation order per (tile_h, tile_w).  float64 in both precisions.
 *   agents[f][s][n]  what dw_download_agents returns for world worlds[s], agent n, on that state: position and energy store
 *                    after step t_f's update_agents (the reference writes the store into channel 4 at that position).
 * At least one of cover, temp_mean and agents is required (records only: dw_run_episode_trace*).  Only the selected worlds
 * produce frames.  A call with neither temps nor temp_mean evaluates no float64 field; one with temp_mean but without
 * temps evaluates it only in frame steps of selected worlds.
 * The forms (dw_kernel_info: "; episode frames: one wave per world" / "launches per step") are dw_run_episode_trace's.
 * H*W <= 256 with at most 64 agents: one wave per world (episode_wave_frames_pw, csrc/dw_episode_wave_frames_pw.hpp: a wave
 * learns from a device map whether its world is selected; in a frame step it adds the cover tiles from the new plane in
 * LDS, sums the staged cell temperatures in dw_reduce_tiles' order and stores its agents, straight into the ring).  Every
 * other shape, DW_NO_EPISODE_WAVE and DW_NO_EPISODE_KERNEL: launches per step, with dw_reduce_tiles' kernels around a frame
 * step.  Both forms return the same bytes.  At most 32 MiB of frame records wait on the device (at least one frame); the
 * wave form splits the call into launches at whole strides whose frames fit, and the ring comes down by stream-ordered
 * copies: there is no other host synchronisation between the steps.
 * Checked before anything is launched or allocated (the state is untouched): the rules of dw_run_episode_trace, those of
 * dw_frame_spec (dw_reduce_tiles), and DW_EINVAL for a null handle, schedule or spec, stride < 1, all three frame outputs
 * null, and agents with n_agents == 0.  DW_ENOMEM keeps nothing.  Synchronises.
 * Out of scope: frames in dw_run_episode_ensemble* and dw_run_episode_mlp*, an LDS workgroup kernel with frames, per-tile
 * extrema, pinned frame arrays. */
typedef struct dw_agent_frame { int32_t row, col; double state; } dw_agent_frame;   /* 16 bytes */
int dw_run_episode_frames(dw_handle* h, int32_t nsteps, const double* L_schedule, int policy_mode,
                          const uint8_t* use_table, const int8_t* table, uint32_t threshold_k,
                          uint8_t* world_alive      /* [K][B], may be NULL */,
                          uint8_t* agent_ok         /* [K][B][N], may be NULL */,
                          dw_world_stats* trace     /* [K][B], may be NULL */,
                          dw_temp_stats* temps      /* [K][B], may be NULL */,
                          const dw_frame_spec* spec, int32_t stride,
                          dw_tile_cover* cover      /* [F][S][TH][TW], may be NULL */,
                          double* temp_mean         /* [F][S][TH][TW], may be NULL */,
                          dw_agent_frame* agents    /* [F][S][N], may be NULL */);

/* ---- plumbing ------------------------------------------------------------------------------- */

/* Use an existing HIP stream (e.g. torch's current stream) instead of the handle's own. */
int dw_set_stream(dw_handle* h, void* hip_stream);
int dw_sync(dw_handle* h);

/* HIP-event timing on the handle's stream: ms between start and stop (stop synchronises). */
int dw_timer_start(dw_handle* h);
int dw_timer_stop(dw_handle* h, float* elapsed_ms);

/* Raw device pointers of the current / previous planes (per-mille binary16, [B][H][W]) for zero-copy interop;
 * DW_ESTATE while the current state is an un-quantised upload (no binary16 planes before the first step). */
int dw_device_planes(dw_handle* h, int which, void** light, void** dark);

/* Name and geometry of the step kernel the handle dispatches for its shape, for bench/profiles:
 * writes a NUL-terminated description into buf.  Appended fragments name the forms of the other entry points:
 * "; trace: ...", "; per-world L: ...", "; ensemble episode: ..." (dw_run_episode_ensemble), "; episode trace: ..."
 * (dw_run_episode_trace), "; episode temperature: ..." (dw_run_episode_trace_temperature), "; ensemble trace: ..."
 * (dw_run_episode_ensemble_trace), "; mlp trace: ..." (dw_run_episode_mlp_trace), behind it "; episode frames: ..."
 * (dw_run_episode_frames), "; mlp counts: workgroup (LDS)" / "launches per step" (dw_run_episode_mlp_counts), and
 * "; episode: F; mlp episode: F" - the form dw_run_episode and
 * dw_run_episode_mlp take for the handle's shape, agent count, precision, collision mode and switches, F one of
 * "one wave per world" (H*W <= 256 and at most 64 agents, MLP: at most 4), "workgroup (LDS)" (H*W <= 4096) and
 * "launches per step" (dw_run_episode_mlp takes its first steps that way until the current and the previous state are
 * quantised, whatever the form). */
int dw_kernel_info(dw_handle* h, char* buf, size_t buflen);

/* Diagnostics for the exact-mode error bound: number of cells re-evaluated in float64 by the last
 * step (summed over worlds). */
int dw_last_fixup_count(dw_handle* h, uint64_t* count);

/* Audit of the exact mode's error bound on the CURRENT (quantised) state at luminosity L: evaluates
 * every cell's per-mille growth in the kernels' float32 arithmetic and in float64 and returns
 *   out[0] max |gq_f32 - gq_f64| in quanta, out[1] max of that error divided by the cell's bound
 *   eps (the bound holds iff < 1), out[2] cells the tie test would flag, out[3] cell-values audited.
 * Used by the tests to show the analytic bound of DESIGN.md is never approached. */
int dw_audit_tie_bound(dw_handle* h, double L, double out[4]);

#ifdef __cplusplus
}
#endif
#endif /* DAISYWORLD_HIP_H */
