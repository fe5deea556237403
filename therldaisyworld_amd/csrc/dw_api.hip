// dw_api.hip — C ABI (include/daisyworld_hip.h) over the gfx950 kernels in dw_kernels.hpp.
//
// Host-side responsibilities: device state (ping-pong binary16 per-mille planes, agents, reductions), the
// launches, and the bookkeeping of the un-quantised initial state (float64 or float32 buffers that live until
// the first step has consumed them).  Which kernels take a step, and the float32 coefficient set derived for it
// from the float64 constants and the current luminosity: dw_plan.hpp.  No CPU compute path exists here.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <optional>
#include <type_traits>
#include <vector>

#include "../../include/daisyworld_hip.h"
#include "dw_kernels.hpp"
#include "dw_host_util.hpp"
#include "dw_plan.hpp"
#include "dw_series.hpp"
#include "dw_episode_staging.hpp"

using namespace dw;

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIPCHK(expr)                                                                           \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(e_ == hipErrorOutOfMemory ? DW_ENOMEM : DW_EHIP, "%s failed: %s (%s:%d)", \
                        #expr, hipGetErrorString(e_), __FILE__, __LINE__);                      \
    } while (0)

#define NEED(cond, code, ...)                      \
    do {                                           \
        if (!(cond)) return fail(code, __VA_ARGS__); \
    } while (0)

// ------------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------------
// An un-quantised state (the reference's initialize_grid does not round, ref :285-324) cannot live in the
// canonical binary16 planes.  It is held in its upload format - float64 natural units (dw_upload_state_f64) or
// float32 per-mille (dw_init_random, dw_upload_state_f32 with quantised = 0) - and is the CURRENT state until
// the first step has read it, then for one more step the PREVIOUS state (observations and the materialised
// grid derive their temperature channels from the pre-step state).  While it is the current state the
// binary16 planes of the `cur` buffer are undefined.
enum UnqKind { UNQ_F64 = 1, UNQ_F32 = 2 };
enum UnqOwner { OWN_NONE = 0, OWN_CUR = 1, OWN_PREV = 2 };

// The handle owns its buffers (dw_host_util.hpp): device memory, and page-locked host memory for the staging images.
// DW_TEST_FAIL_GROUP_ALLOC=<n> (tests, under DW_TEST_HOOKS; process-wide countdown, read when a group is first allocated
// while it is set): the last allocation of each of the next n groups (alloc_group) fails with out-of-memory.  Groups
// that dw_create allocates are not counted.
static thread_local int t_fail_in = 0;     // > 0: the t_fail_in-th device allocation from now fails (armed by alloc_group)
struct DeviceMem {
    static int alloc(void** p, size_t n) {
        if (t_fail_in > 0 && --t_fail_in == 0) return hipErrorOutOfMemory;
        return hipMalloc(p, n);
    }
    static int release(void* p) { return hipFree(p); }
};
struct PinnedMem {
    static int alloc(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
    static int release(void* p) { return hipHostFree(p); }
};
template <class T> using DevBuf = Buf<T, DeviceMem>;
template <class T> using PinnedBuf = Buf<T, PinnedMem>;

struct dw_handle {
    dw_params prm;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    size_t cells = 0;                 // B*H*W
    DevBuf<plane_t> L16[2];           // canonical planes (binary16 per-mille integers), ping-pong
    DevBuf<plane_t> D16[2];
    int cur = 0;
    DevBuf<double> L64;               // un-quantised state, float64 natural units (lazily allocated, kept)
    DevBuf<double> D64;
    DevBuf<float> U32L;               // un-quantised state, float32 per-mille (lazily allocated; freed again
    DevBuf<float> U32D;               //   after use when it is large, see release_unquantised)
    UnqKind unq_kind = UNQ_F64;
    UnqOwner unq = OWN_NONE;
    bool have_state = false;
    bool stepped = false;             // prev/cur form a forward() pair
    double L_last = 0.0;              // luminosity of the last forward()
    bool L_per_world = false;         // ... which took one per world (dw_step_n_trace_per_world): L_last means nothing
    bool P_per_world = false;         // ... and a set of constants per world too (dw_step_n_trace_ensemble): read with L_per_world
    DevBuf<int> idx;                  // [B][N][2]
    DevBuf<double> st;                // [B][N]
    DevBuf<int> action;               // [B][N]
    DevBuf<int> action_tmp;           // staging for host-supplied (possibly sub-shaped) actions
    bool have_agents = false;
    // per-world reductions, double-buffered: each step kernel accumulates into stats2[1-sp] and
    // clears stats2[sp] for the step after it, so the step loop needs no memset launches.
    // Element [B] of each buffer carries the float64 fix-up counter (in sum_l).
    // Each buffer is one allocation: [(B+1) StatsDev][kNumQueues*16 uint queue counters].
    DevBuf<StatsDev> stats2[2];
    size_t stats_bytes = 0;           // bytes of one such buffer
    int sp = 0;                       // buffer holding the CURRENT state's reductions
    DevBuf<uint4> fixq;               // exact mode: global near-tie queues [kNumQueues][qcap][3]
    unsigned int qcap = 0;
    DevBuf<int> redo_tiles;           // exact mode: tiles to recompute whole (queue overflow)
    Switches sw{};                    // experiment / test switches as they were when the handle was created
    StepPlan plan{};                  // kernel selection for `prm`
    DevBuf<int> done_at;              // [B]
    DevBuf<int> agents_done_at;       // [B][N]
    DevBuf<int> n_alive;
    DevBuf<double> scratch;           // device staging for float64 downloads / uploads
    DevBuf<unsigned char> ep_buf;     // device staging of dw_run_episode (schedules, tables, flags)
    DevBuf<double> mlp_w;             // parameter sets of the last dw_run_episode_mlp call that passed them
    int mlp_members = 0;
    DevBuf<int> n_active_d;           // [B] dw_run_episode_mlp_counts: the agents each world has in the call in flight
    PinnedBuf<unsigned char> ep_pinned;   // page-locked host image of ep_buf (LDS-resident episode kernels: ONE upload
                                          // and ONE download per chunk instead of six pageable copies)
    DevBuf<double> reward_d;          // [B][N]
    DevBuf<unsigned char> done_d;     // [B][N]
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t evf0 = nullptr, evf1 = nullptr;   // around the fused launches of the last dw_step_n call
    int fused_launches = 0;           // ... and how many there were (dw_last_step_n_timing); 0 unless BOTH events
                                      // of that call were recorded (an error return in between leaves 0)
    DevBuf<StatsDev> side_stats;      // reductions of dw_forward_f64's side computation (not the handle's)
    DevBuf<StatsDev> trace_d;         // dw_step_n_trace: [rows][B] records of the chunk of steps in flight (grown on demand)
    // dw_reduce_temperature / dw_step_n_trace_temperature: [rows][B] temperature records, and the [B][chunks] partials of
    // the reduction in flight (one group: allocated all or nothing)
    DevBuf<TempStatsDev> temp_d;
    DevBuf<TempPartial> temp_part;
    // dw_reduce_tiles / dw_step_n_frames: the selected worlds [S], the frames that wait for their download (cover records
    // and temperature means, [frames][S][TH][TW] each) and the [S][TH*TW][chunks] partials of large tiles (one group)
    DevBuf<int> frame_sel;
    DevBuf<TileCoverDev> frame_cover;
    DevBuf<double> frame_temp;
    DevBuf<double> tile_part;
    // dw_run_episode_frames: the agents of the frames that wait for their download, [frames][S][N]; in the
    // one-wave-per-world form frame_sel holds every world's place among the selected ones [B] instead of the selection
    DevBuf<AgentFrameDev> frame_agents;
    // dw_step_n_trace_per_world: the constants of a chunk of steps, one entry per step and world (PwLayout), and their
    // page-locked host image
    DevBuf<unsigned char> pw_tab;
    PinnedBuf<unsigned char> pw_pinned;
    PinnedBuf<unsigned char> pinned;  // page-locked host staging of dw_env_step (actions in, obs/reward/done out)
    // dw_snapshot_save[_slot] / dw_snapshot_restore[_slot]: device copies of the current state (two slots: a harness
    // that runs chunk c + 1 while it still accounts for chunk c keeps the starts of both)
    struct Snapshot {
        DevBuf<plane_t> L, D;
        DevBuf<plane_t> PL, PD;       // the retained previous state (observations, caches) when there is one
        bool stepped = false;
        double L_last = 0.0;
        bool L_per_world = false, P_per_world = false;
        UnqOwner unq = OWN_NONE;
        DevBuf<int> idx;
        DevBuf<double> st;
        DevBuf<unsigned char> stats;
        bool valid = false, agents = false;
    } snap[DW_SNAPSHOT_SLOTS];
    // dw_fitness_*: the accumulators of a population's fitness bookkeeping, carried across chunks (one group: sum_reward [P],
    // done_at [B][N], running [P], the three words of a chunk's outcome and their page-locked image), and the scratch of
    // the chunk in flight (a group of its own: means, all-done flags and run_t, [K][P] each).  Not part of the snapshots.
    DevBuf<double> fit_sum;
    DevBuf<int> fit_done_at;
    DevBuf<unsigned char> fit_running;
    DevBuf<int> fit_out;
    PinnedBuf<int> fit_out_host;
    DevBuf<double> fit_means;
    DevBuf<unsigned char> fit_all_done;
    DevBuf<unsigned char> fit_run_t;
    int fit_wpm = 0, fit_half = 0;    // worlds per member and agents per world whose rewards count; 0: no dw_fitness_begin yet
    std::vector<std::pair<const void*, size_t>> lds_limit;   // set_lds_limit: kernel -> dynamic LDS limit set
    bool created = false;             // dw_create has returned it (DW_TEST_FAIL_GROUP_ALLOC counts from then on)
};

static inline bool cur_quantised(const dw_handle* h) { return h->unq != OWN_CUR; }

// After a step the temperature channels of observations and of the materialised grid derive from the pre-step state and
// the luminosity of that step (L_last).  A per-world step has no such number.
static inline bool lacks_shared_L(const dw_handle* h) { return h->stepped && h->L_per_world; }
#define NEED_SHARED_L(h, what)                                                                                          \
    NEED(!lacks_shared_L(h), DW_ESTATE,                                                                                 \
         "%s derives its temperature channels from the last step's luminosity, and the last step "                      \
         "(dw_step_n_trace_per_world) took a per-world luminosity: take a shared-L step or upload a state first", what)
// ... and after dw_step_n_trace_ensemble no single set of constants either: what evaluates the retained state with the
// caller's luminosity and the handle's constants (the caches, their temperature statistics) has nothing to evaluate with
static inline bool lacks_shared_constants(const dw_handle* h) { return lacks_shared_L(h) && h->P_per_world; }
#define NEED_SHARED_CONSTANTS(h, what)                                                                                  \
    NEED(!lacks_shared_constants(h), DW_ESTATE,                                                                         \
         "%s evaluates the last step's input state with one set of constants, and the last step "                       \
         "(dw_step_n_trace_ensemble) took per-world constants: take a shared-L step or upload a state first", what)

// ------------------------------------------------------------------------------------------------
// runtime values -> template arguments.  Each helper instantiates `f` for every value it lists, so it is used only
// where every one of those kernel instantiations is meant to exist.  The helpers, and the launch templates and
// lambdas that use them, deduce their return types: they are instantiated where they are called, so the kernels are
// instantiated - and laid out in the code object - in the order the launch code names them.
// ------------------------------------------------------------------------------------------------
template <int V> using int_c = std::integral_constant<int, V>;

// f(int_c<v>{}) for v among the listed values (the last one takes any other value: the callers pass listed ones only)
template <int V, int... Vs, class F>
static decltype(auto) with_int(int v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) return f(int_c<V>{});
    else return v == V ? f(int_c<V>{}) : with_int<Vs...>(v, f);
}

template <class F>
static decltype(auto) with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

// element type of a plane pointer handed out by with_planes
template <class P> using elem_t = std::remove_cv_t<std::remove_pointer_t<P>>;

// f(light, dark) with the un-quantised state's typed pointers: float64 natural units or float32 per-mille
template <class F>
static decltype(auto) with_unq_planes(const dw_handle* h, F&& f) {
    return h->unq_kind == UNQ_F64 ? f(h->L64.get(), h->D64.get()) : f(h->U32L.get(), h->U32D.get());
}

// ... or, unless `unq`, with the binary16 planes of buffer `buf`
template <class F>
static decltype(auto) with_planes(const dw_handle* h, bool unq, int buf, F&& f) {
    return unq ? with_unq_planes(h, f) : f(h->L16[buf].get(), h->D16[buf].get());
}

// The state observations and the materialised grid derive their temperature channels from: after a step the
// PRE-step state (POST = true), before any step the current one (POST = false).  f(light, dark, POST) with the planes in
// that state's format and POST a bool constant.
template <class F>
static auto with_derived_from(const dw_handle* h, F&& f) {
    const bool post = h->stepped;
    return with_planes(h, h->unq == (post ? OWN_PREV : OWN_CUR), post ? 1 - h->cur : h->cur, [&](auto* L, auto* D) {
        return with_bool(post, [&](auto POST) { return f(L, D, POST); });
    });
}

// Asynchronous copies FROM host memory (the caller's arrays, local vectors) must have finished before that
// memory can go away: a function that issues them declares one of these right after the host buffers, so that
// every early return (HIPCHK / NEED) waits for the stream first.  disarm() after the function's own final
// synchronisation.
struct SyncOnExit {
    hipStream_t stream;
    bool armed = true;
    explicit SyncOnExit(hipStream_t s) : stream(s) {}
    ~SyncOnExit() { if (armed) (void)hipStreamSynchronize(stream); }
    void disarm() { armed = false; }
};

// A failed allocation: clear the sticky error it leaves (it must not poison later checks) and report it.
static int alloc_failed(int rc, const char* what, size_t bytes) {
    (void)hipGetLastError();
    const hipError_t e = static_cast<hipError_t>(rc);
    return fail(e == hipErrorOutOfMemory ? DW_ENOMEM : DW_EHIP, "allocating %s (%zu bytes) failed: %s", what, bytes,
                hipGetErrorString(e));
}
template <class B>
static int reserve(B& buf, const char* what, size_t need, size_t first_size = 0) {
    const int rc = buf.reserve(need, first_size);
    return rc ? alloc_failed(rc, what, need) : DW_OK;
}

// Buffers used together come and go together (dw_host_util.hpp): a failed allocation leaves NONE of them, so a retry on
// the same handle reports DW_ENOMEM again instead of launching on a null buffer.
static int alloc_group(dw_handle* h, const char* what, std::initializer_list<GroupItem<DeviceMem>> group) {
    static int fail_left = -1;                                  // -1: the variable was not set yet
    if (h->created && fail_left < 0)
        if (const char* e = test_hook("DW_TEST_FAIL_GROUP_ALLOC")) fail_left = std::atoi(e);
    const bool armed = h->created && fail_left > 0;
    if (armed) t_fail_in = (int)group.size();
    const int rc = dw::alloc_group(group);
    if (armed && t_fail_in == 0) --fail_left;                  // the injected failure happened (not a complete group)
    t_fail_in = 0;
    size_t bytes = 0;
    for (const auto& g : group) bytes += g.bytes;
    return rc ? alloc_failed(rc, what, bytes) : DW_OK;
}

// the un-quantised float32 buffers are as large as all four canonical planes together: give them back once
// nothing refers to them any more if they are big (the north-star shape: 128 GiB)
static void release_unquantised(dw_handle* h) {
    if (h->unq != OWN_NONE || !h->U32L.get()) return;
    for (const auto& sn : h->snap)
        if (sn.valid && sn.unq == OWN_PREV) return;              // a snapshot's previous state lives there
    if (h->cells * 2 * sizeof(float) < ((size_t)1 << 30)) return;
    (void)hipStreamSynchronize(h->stream);
    h->U32L.reset();
    h->U32D.reset();
}

// The first fused launch of a run ends the life of an un-quantised PREVIOUS state (after it the retained state is two
// steps back anyway): drop it in front of the run, so that release_unquantised's synchronise + free of 128 GiB at the
// north-star shape happen in front of dw_step_n's timed window and not inside it.
static void drop_unquantised_previous(dw_handle* h) {
    if (h->unq == OWN_PREV) { h->unq = OWN_NONE; h->stepped = false; }
    release_unquantised(h);
}

static int ensure_u32(dw_handle* h) {
    const size_t n = sizeof(float) * h->cells;
    return alloc_group(h, "two float32 planes", {{h->U32L, n}, {h->U32D, n}});
}

static int ensure_f64(dw_handle* h) {
    const size_t n = sizeof(double) * h->cells;
    return alloc_group(h, "two float64 planes", {{h->L64, n}, {h->D64, n}});
}

static int run_episode_impl(dw_handle* h, int32_t nsteps, const double* L_schedule, int policy_mode,
                            const uint8_t* use_table, const int8_t* table, uint32_t threshold_k,
                            uint8_t* world_alive, uint8_t* agent_ok, dw_world_stats* trace = nullptr,
                            dw_temp_stats* temps = nullptr);
static bool episode_kernel_applies(const dw_handle* h);
// The form a handle's episode calls take: a pure function of its parameters and switches.  The dispatch of
// run_episode_impl / dw_run_episode_mlp and the text of dw_kernel_info both read these two predicates.
enum EpisodeForm { EPISODE_STEPWISE, EPISODE_WORKGROUP, EPISODE_WAVE };   // launches per step | episode_small / episode_mlp | one wave per world
static EpisodeForm episode_form(const dw_handle* h);
static EpisodeForm episode_mlp_form(const dw_handle* h, size_t* lds_bytes = nullptr);
// dw_run_episode_mlp_counts (dw_counts_plan.hpp): the workgroup kernel, or launches per step
static bool episode_mlp_counts_workgroup(const dw_handle* h) {
    const dw_params& p = h->prm;
    return dw::episode_mlp_counts_workgroup(p.height * p.width, p.n_agents, p.precision == DW_PRECISION_F64, p.collision_mode,
                                            h->sw.no_episode_kernel);
}
// worlds a workgroup of the LDS-resident episode kernels holds (dw_episode.hpp: 256 / wpb threads per world)
static int worlds_per_block(int cells) { return cells <= 256 ? 4 : (cells <= 1024 ? 2 : 1); }
static int observe_into_scratch(dw_handle* h, double L_init, size_t extra_bytes, bool reward_tail = false);

static int ensure_scratch(dw_handle* h, size_t bytes) { return reserve(h->scratch, "scratch", bytes); }

// episode staging buffer (schedules, tables, per-step flags): grown geometrically from 4 MiB so that a
// longer chunk after a short one does not pay a synchronous free + allocation inside a timed run
static int ensure_ep_buf(dw_handle* h, size_t bytes) {
    return reserve(h->ep_buf, "the episode staging buffer", bytes, (size_t)4 << 20);
}

// The host side of an episode call's staging (EpisodeStaging): the handle's device buffer and, staged, its page-locked
// image - the inputs go up in ONE copy, flags and records come back in ONE (round 3: four pageable uploads, a memset and
// two pageable downloads - 88 us of host time per 64-step chunk of 1000 8x8 worlds against 116 us of kernel).  A direct
// call (beyond 64 MiB; the launches per step, whose only input is the table) copies each region straight from / to the
// caller's arrays.  Declare it in front of the call's SyncOnExit: uploads read its vectors.
struct EpisodeBuffers {
    using R = EpisodeStaging;
    dw_handle* h;
    const EpisodeStaging S;
    unsigned char* img = nullptr;
    std::vector<PhysF32> p32_own;                               // (direct calls)
    std::vector<unsigned char> ut_own;

    EpisodeBuffers(dw_handle* h_, const EpisodeStaging& S_) : h(h_), S(S_) {}
    bool out_direct = false;                                    // the image holds the inputs only: finish() copies as a direct call
    // `inputs_only` (staged): the image ends where the device's outputs begin - uploads as staged, finish() straight to
    // the caller's arrays (dw_run_episode_ensemble_trace beyond fits_image(): its records alone may be hundreds of MB)
    int alloc(bool staged, bool inputs_only = false) {
        if (int rc = ensure_ep_buf(h, S.total)) return rc;
        if (!staged) return DW_OK;
        const size_t image = inputs_only ? S.off[R::WORLD_ALIVE] : S.total;
        if (int rc = reserve(h->ep_pinned, "the page-locked episode staging", image, (size_t)1 << 20)) return rc;
        img = h->ep_pinned.get();
        out_direct = inputs_only;
        return DW_OK;
    }
    template <class T = unsigned char>
    T* dev(R::Region r) const { return S.at<T>(h->ep_buf.get(), r); }
    // where the caller derives the float32 rows of the next upload
    PhysF32* p32() {
        if (img) return S.at<PhysF32>(img, R::P32);
        p32_own.resize(S.bytes[R::P32] / sizeof(PhysF32));
        return p32_own.data();
    }
    // the rows in p32(), `n_ls` luminosities; `first`: also P64 as the caller wrote it, use_table (null: zeros) and the table
    int upload(const double* Ls, size_t n_ls, bool first, const uint8_t* use_table, const int8_t* table) {
        const bool have_table = table && S.bn;
        const size_t ut_bytes = S.bytes[R::USE_TABLE];
        auto to_dev = [&](R::Region r, const void* src, size_t bytes) {
            return bytes ? hipMemcpyAsync(dev(r), src, bytes, hipMemcpyHostToDevice, h->stream) : hipSuccess;
        };
        if (img) {
            std::memcpy(img + S.off[R::LS], Ls, sizeof(double) * n_ls);
            if (first) {
                if (use_table) std::memcpy(img + S.off[R::USE_TABLE], use_table, ut_bytes);
                else std::memset(img + S.off[R::USE_TABLE], 0, ut_bytes);
                if (have_table) std::memcpy(img + S.off[R::TABLE], table, S.bytes[R::TABLE]);
            }
            const size_t upto = first ? S.input_end(have_table) : S.off[R::LS] + sizeof(double) * n_ls;
            HIPCHK(hipMemcpyAsync(h->ep_buf.get(), img, upto, hipMemcpyHostToDevice, h->stream));
            return DW_OK;
        }
        HIPCHK(to_dev(R::P32, p32_own.data(), S.bytes[R::P32]));
        HIPCHK(to_dev(R::LS, Ls, sizeof(double) * n_ls));
        if (ut_bytes) {
            ut_own.assign(ut_bytes, 0);
            if (use_table) std::memcpy(ut_own.data(), use_table, ut_bytes);
            HIPCHK(to_dev(R::USE_TABLE, ut_own.data(), ut_bytes));
        }
        if (have_table) HIPCHK(to_dev(R::TABLE, table, S.bytes[R::TABLE]));
        return DW_OK;
    }
    // flags and records come back (staged: the one span that covers what the caller wants), the stream is synchronised
    // (`temps`: the second block of TRACE, behind the records)
    int finish(uint8_t* world_alive, uint8_t* agent_ok, dw_world_stats* trace, dw_temp_stats* temps = nullptr) {
        if (!S.bn) agent_ok = nullptr;
        struct { void* dst; size_t off, bytes; } out[4] = {{world_alive, S.off[R::WORLD_ALIVE], S.bytes[R::WORLD_ALIVE]},
                                                           {agent_ok, S.off[R::AGENT_OK], S.bytes[R::AGENT_OK]},
                                                           {trace, S.off[R::TRACE], S.stats_bytes},
                                                           {temps, S.temps_off(), S.temps_bytes}};
        const bool staged = img && !out_direct;
        size_t lo = S.total, hi = 0;
        for (const auto& o : out) {
            if (!o.dst) continue;
            if (!staged) HIPCHK(hipMemcpyAsync(o.dst, h->ep_buf.get() + o.off, o.bytes, hipMemcpyDeviceToHost, h->stream));
            lo = o.off < lo ? o.off : lo;
            hi = o.off + o.bytes > hi ? o.off + o.bytes : hi;
        }
        if (staged && hi > lo) HIPCHK(hipMemcpyAsync(img + lo, h->ep_buf.get() + lo, hi - lo, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (staged)
            for (const auto& o : out)
                if (o.dst) std::memcpy(o.dst, img + o.off, o.bytes);
        return DW_OK;
    }
};

// What the LDS-resident episode launches pass alike (EpisodeIO and EpisodeMlpIO): the planes in place, the agents, the
// reductions of the current state, and the float32 sets and luminosities of the steps in the staging buffer
template <class IO>
static void fill_episode_io(IO& io, const dw_handle* h, const EpisodeStaging& S) {
    const int cur = h->cur, prev = 1 - h->cur;
    io.L = h->L16[cur].get(); io.D = h->D16[cur].get(); io.prevL = h->L16[prev].get(); io.prevD = h->D16[prev].get();
    io.idx = h->idx.get(); io.st = h->st.get();
    io.P32 = S.at<const PhysF32>(h->ep_buf.get(), EpisodeStaging::P32);
    io.Ls = S.at<const double>(h->ep_buf.get(), EpisodeStaging::LS);
    io.stats = h->stats2[h->sp].get();
    io.fixups = &io.stats[h->prm.batch].sum_l;
}

// Dynamic LDS above the default limit: the attribute belongs to the device's copy of the kernel (a handle is bound to
// one device), so the handle remembers the largest value it set per kernel and sets it again only to raise it.
template <class Kernel>
static int set_lds_limit(dw_handle* h, Kernel kern, size_t bytes) {
    const void* k = reinterpret_cast<const void*>(kern);
    size_t* set = nullptr;
    for (auto& e : h->lds_limit)
        if (e.first == k) set = &e.second;
    if (set && *set >= bytes) return DW_OK;
    HIPCHK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    if (set) *set = bytes;
    else h->lds_limit.emplace_back(k, bytes);
    return DW_OK;
}

// near-tie queues of the tiled exact kernel (the streaming kernel keeps them in LDS) when `plan` needs them: room for 1/64
// of all cells (the bound flags ~0.3-0.5 %), at least 2048 entries per queue; 48 bytes per entry, i.e. 0.75 B per cell
// on top of the 16 B of state
static int ensure_fixq(dw_handle* h, const StepPlan& plan) {
    if (!plan.need_fixq) return DW_OK;
    const dw_params& p = h->prm;                                // (the shape: the same for every plan of a handle)
    size_t per_q = (h->cells / 64 + kNumQueues - 1) / kNumQueues;
    if (per_q < 2048) per_q = 2048;
    per_q = (per_q + 255) / 256 * 256;
    const size_t max_tiles = (size_t)p.batch * ((p.height + 7) / 8) * ((p.width / 4 + 15) / 16);
    if (int rc = alloc_group(h, "the near-tie queues", {{h->fixq, sizeof(uint4) * 3 * per_q * kNumQueues},
                                                         {h->redo_tiles, sizeof(int) * max_tiles}}))
        return rc;
    h->qcap = (unsigned int)per_q;
    return DW_OK;
}

// What every step launch passes besides its input planes
struct StepOut {
    plane_t* L; plane_t* D;                   // the binary16 planes of the other buffer
    PhysF32 P;                                // the constants of a single step at one luminosity (launch_forward) ...
    PhysF64 P64;
    StatsDev* stats;                          // the new state's reductions (all zero before the step) ...
    unsigned long long* fixups;               // ... and the float64 fix-up counter behind them
    unsigned long long* zero_me;              // the old state's reductions: cleared for the step after this one
    int zero_n;
};
// ... all of it but the constants
static StepOut step_out(const dw_handle* h) {
    const int out = 1 - h->cur;
    StatsDev* stats = h->stats2[1 - h->sp].get();                       // invariant: all zero
    return StepOut{h->L16[out].get(), h->D16[out].get(), PhysF32{}, PhysF64{}, stats, &stats[h->prm.batch].sum_l,
                   reinterpret_cast<unsigned long long*>(h->stats2[h->sp].get()),
                   (int)(h->stats_bytes / sizeof(unsigned long long))};
}

template <int TCQ, int RPT, bool EXACT>
static int launch_tiled(dw_handle* h, const plane_t* iL, const plane_t* iD, const StepOut& o, const FixQ& fq) {
    auto kern = step_tiled<TCQ, RPT, EXACT>;
    // only the 32-row tuning tiles exceed the 64 KB a launch may ask for without opting in
    if constexpr (TileCfg<TCQ, RPT>::LDS_BYTES > 64 * 1024)
        if (int rc = set_lds_limit(h, kern, TileCfg<TCQ, RPT>::LDS_BYTES)) return rc;
    const Geom& g = h->plan.geom;
    constexpr size_t lds_bytes = TileCfg<TCQ, RPT>::LDS_BYTES;
    hipLaunchKernelGGL(kern, dim3((unsigned)g.chunk * 8u), dim3(256), lds_bytes, h->stream, iL, iD, o.L, o.D, g, o.P, o.stats,
                       o.fixups, o.zero_me, o.zero_n, fq);
    HIPCHK(hipGetLastError());
    if (EXACT) {
        // second kernel of the step: dense float64 re-evaluation of the queued near-tie cells
        const dim3 qg((fq.qcap + 255) / 256, kNumQueues);
        hipLaunchKernelGGL(fixup_cells, qg, dim3(256), 0, h->stream, o.L, o.D, h->prm.height, h->prm.width, o.P64, o.stats, fq);
        // third: whole tiles whose queue overflowed (normally none: exits immediately)
        hipLaunchKernelGGL(redo_tiles_f64, dim3(256), dim3(256), 0, h->stream, iL, iD, o.L, o.D, g, TileCfg<TCQ, RPT>::TR, TCQ,
                           o.P64, o.stats, fq);
        HIPCHK(hipGetLastError());
    }
    return DW_OK;
}

// The kernels that take their world from blockIdx.y - one thread per cell, or a chunk of cells per workgroup - are launched
// on grids (x, worlds), and a grid holds 65 535 workgroups in y: an ensemble of more worlds goes in slices of that many,
// f(b0, nb) for the worlds [b0, b0 + nb).  f advances every per-world address by b0 itself (planes by b0 * H * W cells,
// tables and records by b0 entries), so the kernels see a batch of nb worlds and index inside the slice as ever.
constexpr int kGridWorlds = 65535;
template <class F>
static void for_world_slices(int batch, F&& f) {
    for (int b0 = 0; b0 < batch; b0 += kGridWorlds) f(b0, batch - b0 < kGridWorlds ? batch - b0 : kGridWorlds);
}

// one thread per cell (several for big jobs: *cpt): the x extent of the grid of step_generic / step_generic_pw
static unsigned generic_grid_x(const dw_params& p, int* cpt) {
    *cpt = generic_cells_per_thread(p.batch, (long long)p.height * p.width);
    return (unsigned)(((long long)p.height * p.width + 256LL * *cpt - 1) / (256LL * *cpt));
}

// ... any input format
template <class T, int PREC>
static auto launch_generic(dw_handle* h, const T* iL, const T* iD, const StepOut& o, const FirstStepBound& fb = {}) {
    const dw_params& p = h->prm;
    int cpt;
    const unsigned gx = generic_grid_x(p, &cpt);
    const size_t n = (size_t)p.height * p.width;
    for_world_slices(p.batch, [&](int b0, int nb) {               // (every slice clears zero_me: the same zeros again)
        const size_t w = (size_t)b0 * n;
        hipLaunchKernelGGL((step_generic<T, PREC>), dim3(gx, (unsigned)nb), dim3(256), 0, h->stream, iL + w, iD + w, o.L + w,
                           o.D + w, p.height, p.width, o.P, o.P64, o.stats + b0, o.fixups, o.zero_me, o.zero_n, cpt, fb);
    });
}

// the materialise launches of a batch: [B][7], [B][3], [B][3], [B][2] and [B] planes out (null: not wanted)
template <class PrevT, bool POST>
static void launch_materialise(dw_handle* h, const PrevT* pL, const PrevT* pD, const plane_t* cL, const plane_t* cD,
                               const PhysF64& P, double* grid7, double* temps, double* betas, double* growth, double* teff) {
    const dw_params& p = h->prm;
    const size_t n = (size_t)p.height * p.width;
    auto at = [](double* q, size_t off) { return q ? q + off : q; };
    for_world_slices(p.batch, [&](int b0, int nb) {
        const size_t w = (size_t)b0 * n;
        hipLaunchKernelGGL((materialise<PrevT, POST>), dim3((unsigned)((n + 255) / 256), (unsigned)nb), dim3(256), 0, h->stream,
                           pL + w, pD + w, cL + w, cD + w, p.height, p.width, P, at(grid7, 7 * w), at(temps, 3 * w),
                           at(betas, 3 * w), at(growth, 2 * w), at(teff, w));
    });
}

// the first step from the un-quantised state, read in its upload format (StepPlan::first_prec, first_stream)
static int launch_first_step(dw_handle* h, double L, const StepOut& o) {
    const StepPlan& pl = h->plan;
    const FirstStepBound fb = pl.first_prec == 3 ? derive_first_bound(h->prm, L, o.P, h->unq_kind == UNQ_F64, h->sw.first_slack)
                                                 : FirstStepBound{};
    if (pl.first_stream) {
        const dim3 grid((unsigned)((pl.first_geom.nstrips + 3) / 4));
        with_unq_planes(h, [&](auto* iL, auto* iD) {
            with_int<1, 3>(pl.first_prec, [&](auto PR) {
                with_int<0, 1, 2, 3>(pl.halo, [&](auto HL) {
                    hipLaunchKernelGGL((step_first_stream<elem_t<decltype(iL)>, PR, HL>), grid, dim3(256), 0, h->stream, iL, iD,
                                       o.L, o.D, pl.first_geom, o.P, o.P64, o.stats, o.fixups, o.zero_me, o.zero_n, fb);
                });
            });
        });
    } else {
        with_unq_planes(h, [&](auto* iL, auto* iD) {
            with_int<1, 3, 2>(pl.first_prec, [&](auto PR) { launch_generic<elem_t<decltype(iL)>, PR>(h, iL, iD, o, fb); });
        });
    }
    HIPCHK(hipGetLastError());
    return DW_OK;
}

// a step from the binary16 planes of `cur` by the plan's kernel
static int launch_step(dw_handle* h, const StepOut& o) {
    const dw_params& p = h->prm;
    const StepPlan& pl = h->plan;
    const plane_t* iL = h->L16[h->cur].get();
    const plane_t* iD = h->D16[h->cur].get();
    const bool ex = p.precision == DW_PRECISION_EXACT;
    if (pl.kind == STEP_GENERIC) {                              // PREC 0 exact, 1 fast, 2 f64
        const int prec = p.precision == DW_PRECISION_F64 ? 2 : (ex ? 0 : 1);
        with_int<2, 0, 1>(prec, [&](auto PR) { launch_generic<plane_t, PR>(h, iL, iD, o); });
    } else if (pl.kind == STEP_STREAM && ex) {
        const StreamExactArgs A{iL, iD, o.L, o.D, pl.sgeom, o.P, o.stats, o.fixups, o.zero_me, o.zero_n, o.P64};
        with_int<0, 1, 2, 3>(pl.halo, [&](auto HL) {
            with_bool(pl.sym_albedo, [&](auto SYM) {
                hipLaunchKernelGGL((step_stream_exact<HL, SYM>), dim3((unsigned)pl.sgeom.chunk * 8u), dim3(256), 0, h->stream, A);
            });
        });
    } else if (pl.kind == STEP_STREAM) {
        with_int<0, 1, 2, 3>(pl.halo, [&](auto HL) {
            hipLaunchKernelGGL((step_stream_fast<HL>), dim3((unsigned)pl.sgeom.chunk * 8u), dim3(256), 0, h->stream, iL, iD, o.L,
                               o.D, pl.sgeom, o.P, o.P64, o.stats, o.fixups, o.zero_me, o.zero_n);
        });
    } else {
        FixQ fq;
        fq.entries = h->fixq.get();
        fq.counts = reinterpret_cast<unsigned int*>(o.stats + p.batch + 1);
        fq.qcap = h->qcap;
        fq.redo_tiles = h->redo_tiles.get();
        auto tiled = [&](auto TCQ, auto RPT) {
            return with_bool(ex, [&](auto EX) { return launch_tiled<TCQ, RPT, EX>(h, iL, iD, o, fq); });
        };
        // the tile shapes plan_steps picks: TCQ 64 with RPT 4 (8 or 2 under DW_TILE_RPT), 32 x 4, 16 x 2
        if (pl.tcq == 64) return with_int<8, 4, 2>(pl.rpt, [&](auto RPT) { return tiled(int_c<64>{}, RPT); });
        return pl.tcq == 32 ? tiled(int_c<32>{}, int_c<4>{}) : tiled(int_c<16>{}, int_c<2>{});
    }
    HIPCHK(hipGetLastError());
    return DW_OK;
}

// A step wrote the other buffer: it holds the current state now, and the reductions swap with it.
static void step_done(dw_handle* h, double L, bool stepped, bool per_world = false, bool per_world_constants = false) {
    h->cur = 1 - h->cur;
    h->sp = 1 - h->sp;
    h->unq = h->unq == OWN_CUR ? OWN_PREV : OWN_NONE;
    h->stepped = stepped;
    h->L_last = L;
    h->L_per_world = per_world;
    h->P_per_world = per_world && per_world_constants;
    release_unquantised(h);
}

// An episode kernel stepped the current buffer in place and left the state before its last step in the other one: a
// forward() pair at L_last, or (`per_world`: episode_wave_pw) per-world in both senses, as after dw_step_n_trace_ensemble.
static void episode_done(dw_handle* h, double L_last, bool per_world) {
    h->unq = OWN_NONE;
    h->stepped = true;
    h->L_last = per_world ? 0.0 : L_last;
    h->L_per_world = per_world;
    h->P_per_world = per_world;
}

// forward(): cur -> other buffer, swap.  Assumes agents were already updated.
static int launch_forward(dw_handle* h, double L) {
    const dw_params& p = h->prm;
    NEED(h->have_state, DW_ESTATE, "no state uploaded (call dw_upload_state_* or dw_init_random)");
    StepOut o = step_out(h);
    o.P = derive_f32(p, L);
    o.P64 = make_f64(p, L);
#ifdef DW_TUNING
    if (const char* e = std::getenv("DW_ABLATE")) {
        if (std::strcmp(e, "copy") == 0) {
            const int in = h->cur;
            const size_t n4 = h->cells * sizeof(plane_t) / 16;
            hipLaunchKernelGGL(copy_planes, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, h->stream,
                               reinterpret_cast<const float4*>(h->L16[in].get()), reinterpret_cast<const float4*>(h->D16[in].get()),
                               reinterpret_cast<float4*>(o.L), reinterpret_cast<float4*>(o.D), n4);
            HIPCHK(hipGetLastError());
            step_done(h, L, true);
            return DW_OK;
        }
        const int v = std::strcmp(e, "nomath") == 0 ? 1 : 0;
        HIPCHK(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_ablate), &v, sizeof(int), 0, hipMemcpyHostToDevice, h->stream));
    }
#endif
    if (int rc = h->unq == OWN_CUR ? launch_first_step(h, L, o) : launch_step(h, o)) return rc;
    step_done(h, L, true);
    return DW_OK;
}

// ---- per-world luminosities and constants (dw_step_n_trace_per_world, dw_step_n_trace_ensemble) ----------------------
// One step, world b with the constants row32[b] / row64[b] (device addresses): the first step from an un-quantised state
// and every shape the per-world wave-strip kernels do not take by step_generic_pw.
// `sym`: the albedo-symmetric form of the exact wave-strip kernel (every world's set is symmetric); `constants`: the rows
// differ in more than the luminosity (dw_step_n_trace_ensemble), which the handle remembers.
static int launch_forward_pw(dw_handle* h, const PhysF32* row32, const PhysF64* row64, const FirstStepBound* rowfb, bool sym,
                             bool constants) {
    const dw_params& p = h->prm;
    const StepPlan& pl = h->plan;
    const StepOut o = step_out(h);                              // (its constants stay unset: the rows carry them)
    const bool ex = p.precision == DW_PRECISION_EXACT;
    auto generic = [&](auto* iL, auto* iD, auto PR) {
        int cpt;
        const unsigned gx = generic_grid_x(p, &cpt);
        const size_t n = (size_t)p.height * p.width;
        for_world_slices(p.batch, [&](int b0, int nb) {
            const size_t w = (size_t)b0 * n;
            hipLaunchKernelGGL((step_generic_pw<elem_t<decltype(iL)>, PR>), dim3(gx, (unsigned)nb), dim3(256), 0, h->stream,
                               iL + w, iD + w, o.L + w, o.D + w, p.height, p.width, row32 + b0, row64 + b0,
                               rowfb ? rowfb + b0 : rowfb, o.stats + b0, o.fixups, o.zero_me, o.zero_n, cpt);
        });
    };
    const plane_t* iL = h->L16[h->cur].get();
    const plane_t* iD = h->D16[h->cur].get();
    if (h->unq == OWN_CUR) {                                    // PREC as launch_first_step: 1 float32, 3 bounded, 2 float64
        with_unq_planes(h, [&](auto* uL, auto* uD) {
            with_int<1, 3, 2>(pl.first_prec, [&](auto PR) { generic(uL, uD, PR); });
        });
    } else if (pl.pw_stream && ex) {
        const StreamExactPwArgs A{iL, iD, o.L, o.D, pl.sgeom, row32, row64, o.stats, o.fixups, o.zero_me, o.zero_n};
        with_int<0, 1, 2>(pl.halo, [&](auto HL) {
            with_bool(sym, [&](auto SYM) {
                hipLaunchKernelGGL((step_stream_exact_pw<HL, SYM>), dim3((unsigned)pl.sgeom.chunk * 8u), dim3(256), 0, h->stream, A);
            });
        });
    } else if (pl.pw_stream) {
        with_int<0, 1, 2>(pl.halo, [&](auto HL) {
            hipLaunchKernelGGL((step_stream_fast_pw<HL>), dim3((unsigned)pl.sgeom.chunk * 8u), dim3(256), 0, h->stream, iL, iD, o.L,
                               o.D, pl.sgeom, row32, row64, o.stats, o.fixups, o.zero_me, o.zero_n);
        });
    } else {                                                    // PREC 0 exact, 1 fast, 2 f64
        const int prec = p.precision == DW_PRECISION_F64 ? 2 : (ex ? 0 : 1);
        with_int<2, 0, 1>(prec, [&](auto PR) { generic(iL, iD, PR); });
    }
    HIPCHK(hipGetLastError());
    step_done(h, 0.0, true, true, constants);
    return DW_OK;
}

// Two steps in one launch, world b with the coefficient sets row[b] (a device address): the trace form of the float32-only
// step pairs (launch_forward_fused2 with `trace`) on the plan's un-packed overlapped or rotating strips.  The retained
// previous state is not valid afterwards; the caller ends with a single step.
static int launch_forward_fused2_pw(dw_handle* h, const PairPw* row, StatsDev* trace) {
    const StepPlan& pl = h->plan;
    const StepOut o = step_out(h);                              // (its constants stay unset: the row carries them)
    const FusedGeom& g = pl.fgeom;
    const dim3 grid((unsigned)g.chunk * 8u);
    const plane_t *inL = h->L16[h->cur].get(), *inD = h->D16[h->cur].get();
    with_int<kFusedRot, kFusedOvl>(pl.fused_mode, [&](auto MODE) {
        hipLaunchKernelGGL((trace_pair_fast_pw<MODE>), grid, dim3(256), 0, h->stream, inL, inD, o.L, o.D, g, row, o.zero_me,
                           o.zero_n, trace);
    });
    HIPCHK(hipGetLastError());
    step_done(h, 0.0, false, true, true);
    return DW_OK;
}

// ---- per-world temperature statistics (dw_reduce_temperature, dw_step_n_trace_temperature) ---------------------------
static int temp_chunks(const dw_handle* h) {
    return (int)(((long long)h->prm.height * h->prm.width + kTempChunk - 1) / kTempChunk);
}
static size_t temp_part_bytes(const dw_handle* h) { return sizeof(TempPartial) * (size_t)h->prm.batch * temp_chunks(h); }

// The statistics of the temperature field a step at luminosity L computes from the CURRENT state (`current`: the trace
// loop, in front of the step) or of the field the caches hold (the state with_derived_from names), into out[B] on the
// device.  row64 != null: world b at the constants row64[b] (a row of the per-world table) instead of L.
static int launch_temp_moments(dw_handle* h, bool current, double L, const PhysF64* row64, TempStatsDev* out) {
    const dw_params& p = h->prm;
    const int chunks = temp_chunks(h);
    const PhysF64 P = row64 ? PhysF64{} : make_f64(p, L);
    TempPartial* part = h->temp_part.get();
    auto reduce = [&](auto* iL, auto* iD) {
        with_bool(row64 != nullptr, [&](auto TABLE) {
            for_world_slices(p.batch, [&](int b0, int nb) {
                const size_t w = (size_t)b0 * p.height * p.width;
                hipLaunchKernelGGL((temp_moments_pw<elem_t<decltype(iL)>, TABLE>), dim3((unsigned)chunks, (unsigned)nb), dim3(256),
                                   0, h->stream, iL + w, iD + w, p.height, p.width, P, row64 ? row64 + b0 : row64,
                                   part + (size_t)b0 * chunks);
            });
        });
    };
    if (current) with_planes(h, h->unq == OWN_CUR, h->cur, reduce);
    else with_derived_from(h, [&](auto* iL, auto* iD, auto) { reduce(iL, iD); });
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(temp_moments_finish_pw, dim3((unsigned)((p.batch + 63) / 64)), dim3(64), 0, h->stream, part, p.batch, chunks,
                       (double)p.height * (double)p.width, out);
    HIPCHK(hipGetLastError());
    return DW_OK;
}

// ---- spatial frames (dw_reduce_tiles, dw_step_n_frames) --------------------------------------------------------------
// A checked dw_frame_spec: the tile geometry, the selection (`listed`: frame_sel holds it; otherwise world s is s), which
// mapping reduces a tile's temperatures (a function of the tile's cells alone, dw_tile_maps.hpp) and the sizes.
struct FrameShape {
    TileGeom G{};
    int S = 0;
    bool listed = false;
    const int32_t* worlds = nullptr;  // the caller's list (uploaded by upload_selection)
    size_t tiles = 0;                 // per world
    int map = 0;
    bool vec8 = false;                // tile_cover_pw<8> applies
    size_t records() const { return (size_t)S * tiles; }                        // of one frame, each of 8 bytes
    size_t part_bytes() const { return G.chunks > 1 ? sizeof(double) * records() * (size_t)G.chunks : 0; }
    size_t sel_bytes() const { return listed ? sizeof(int) * (size_t)S : 0; }
};

static int check_frame_spec(const dw_handle* h, const dw_frame_spec* spec, FrameShape* out) {
    const dw_params& p = h->prm;
    NEED(spec->tile_h >= 1 && spec->tile_w >= 1 && p.height % spec->tile_h == 0 && p.width % spec->tile_w == 0, DW_EINVAL,
         "a %d x %d tile does not divide the %d x %d grid", spec->tile_h, spec->tile_w, p.height, p.width);
    const long long n = (long long)spec->tile_h * spec->tile_w;
    NEED(n <= (1LL << 20), DW_EINVAL, "a %d x %d tile has more than 1 048 576 cells (its per-mille sums would not fit 32 bits)",
         spec->tile_h, spec->tile_w);
    NEED(spec->n_worlds >= 0, DW_EINVAL, "n_worlds < 0");
    NEED(spec->n_worlds == 0 || spec->worlds, DW_EINVAL, "n_worlds > 0 with a null list of worlds");
    std::vector<unsigned char> seen(spec->n_worlds ? (size_t)p.batch : 0, 0);
    for (int32_t i = 0; i < spec->n_worlds; ++i) {
        const int32_t b = spec->worlds[i];
        NEED(b >= 0 && b < p.batch, DW_EINVAL, "worlds[%d] = %d is not a world of this handle (0..%d)", i, b, p.batch - 1);
        NEED(!seen[(size_t)b], DW_EINVAL, "worlds[%d] = %d is listed twice", i, b);
        seen[(size_t)b] = 1;
    }
    FrameShape s;
    TileGeom& G = s.G;
    G.H = p.height, G.W = p.width, G.th = spec->tile_h, G.tw = spec->tile_w, G.TH = G.H / G.th, G.TW = G.W / G.tw;
    for (G.rpt = G.th < 16 ? G.th : 16; G.th % G.rpt; --G.rpt) {}
    s.map = n <= kTileThreadCells ? 0 : (n <= kTileWaveCells ? 1 : 2);
    G.chunks = s.map == 2 ? (int)((n + kTileChunk - 1) / kTileChunk) : 1;
    s.listed = spec->n_worlds > 0;
    s.worlds = spec->worlds;
    s.S = s.listed ? spec->n_worlds : p.batch;
    s.tiles = (size_t)G.TH * G.TW;
    s.vec8 = G.W % 8 == 0 && (G.tw % 8 == 0 || 8 % G.tw == 0);
    *out = s;
    return DW_OK;
}
static int check_luminosity(double L, long long t) {
    NEED(std::isfinite(L) && L >= 0.0, DW_EINVAL, "L[step %lld] = %g: a luminosity is finite and not negative", t, L);
    return DW_OK;
}

static int upload_selection(dw_handle* h, const FrameShape& s) {
    if (s.listed) HIPCHK(hipMemcpyAsync(h->frame_sel.get(), s.worlds, s.sel_bytes(), hipMemcpyHostToDevice, h->stream));
    return DW_OK;
}

// the tile sums of the binary16 planes of buffer `buf` into rec[S][TH][TW]
static int launch_tile_cover(dw_handle* h, const FrameShape& s, int buf, TileCoverDev* rec) {
    const TileGeom& G = s.G;
    const int* sel = s.listed ? h->frame_sel.get() : nullptr;
    HIPCHK(hipMemsetAsync(rec, 0, sizeof(TileCoverDev) * s.records(), h->stream));   // (the kernel adds: integers, any order)
    with_bool(s.vec8, [&](auto V8) {
        constexpr int VEC = V8 ? 8 : 1;
        const unsigned gx = (unsigned)(((long long)(G.H / G.rpt) * (G.W / VEC) + 255) / 256);
        for_world_slices(s.S, [&](int s0, int ns) {
            hipLaunchKernelGGL((tile_cover_pw<VEC>), dim3(gx, (unsigned)ns), dim3(256), 0, h->stream, h->L16[buf].get(),
                               h->D16[buf].get(), G, sel, s0, rec);
        });
    });
    HIPCHK(hipGetLastError());
    return DW_OK;
}

// The tile means of the temperature field a step at luminosity L computes from the CURRENT state (`current`: the frame
// steps, in front of the step) or of the field the caches hold (the state with_derived_from names), into mean[S][TH][TW]
static int launch_tile_temp(dw_handle* h, bool current, double L, const FrameShape& s, double* mean) {
    const TileGeom& G = s.G;
    const PhysF64 P = make_f64(h->prm, L);
    const int* sel = s.listed ? h->frame_sel.get() : nullptr;
    double* part = h->tile_part.get();
    const unsigned gx = s.map == 0 ? (unsigned)((s.tiles + 255) / 256) : (s.map == 1 ? (unsigned)((s.tiles + 3) / 4)
                                                                                      : (unsigned)(s.tiles * (size_t)G.chunks));
    auto reduce = [&](auto* iL, auto* iD) {
        with_int<0, 1, 2>(s.map, [&](auto MAP) {
            for_world_slices(s.S, [&](int s0, int ns) {
                hipLaunchKernelGGL((tile_temp_pw<elem_t<decltype(iL)>, MAP>), dim3(gx, (unsigned)ns), dim3(256), 0, h->stream, iL,
                                   iD, G, P, sel, s0, mean, part);
            });
        });
    };
    if (current) with_planes(h, h->unq == OWN_CUR, h->cur, reduce);
    else with_derived_from(h, [&](auto* iL, auto* iD, auto) { reduce(iL, iD); });
    HIPCHK(hipGetLastError());
    if (G.chunks > 1) {
        hipLaunchKernelGGL(tile_temp_finish_pw, dim3((unsigned)((s.records() + 255) / 256)), dim3(256), 0, h->stream, part,
                           s.records(), G.chunks, (double)G.th * (double)G.tw, mean);
        HIPCHK(hipGetLastError());
    }
    return DW_OK;
}

// The frames of one dw_step_n_frames or dw_run_episode_frames call: they wait in a ring of `cap` frames on the device
// (32 MiB of records, at least one frame) and come down when it is full and at the end of the run.
struct FrameRun {
    dw_handle* h;
    FrameShape sh;
    int stride;
    dw_tile_cover* cover;             // the caller's arrays [F][S][TH][TW] (either may be null)
    double* temp;
    dw_agent_frame* agents = nullptr; // dw_run_episode_frames: the caller's [F][S][N] (may be null)
    size_t total = 0, cap = 1, done = 0;
    size_t agent_records() const { return (size_t)sh.S * (size_t)h->prm.n_agents; }   // of one frame, each of 16 bytes
    void plan(size_t nframes) {
        const size_t bytes = sh.records() * ((cover ? sizeof(TileCoverDev) : 0) + (temp ? sizeof(double) : 0)) +
                             (agents ? sizeof(AgentFrameDev) * agent_records() : 0);
        total = nframes;
        cap = h->sw.frame_ring >= 1 ? (size_t)h->sw.frame_ring : ((size_t)32 << 20) / bytes;
        cap = cap < 1 ? 1 : cap;
        cap = cap > total ? total : cap;                        // (a run without a frame holds none)
    }
    size_t cover_bytes() const { return cover ? sizeof(TileCoverDev) * cap * sh.records() : 0; }
    size_t temp_bytes() const { return temp ? sizeof(double) * cap * sh.records() : 0; }
    size_t agents_bytes() const { return agents ? sizeof(AgentFrameDev) * cap * agent_records() : 0; }
    // the first `k` frames of the ring are frames f0 .. f0 + k - 1 of the call: down to the caller's arrays, on the stream
    int download(size_t f0, size_t k) {
        const size_t at = f0 * sh.records(), n = k * sh.records();
        if (cover && n) HIPCHK(hipMemcpyAsync(cover + at, h->frame_cover.get(), sizeof(TileCoverDev) * n, hipMemcpyDeviceToHost, h->stream));
        if (temp && n) HIPCHK(hipMemcpyAsync(temp + at, h->frame_temp.get(), sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
        if (agents && k)
            HIPCHK(hipMemcpyAsync(agents + f0 * agent_records(), h->frame_agents.get(), sizeof(AgentFrameDev) * k * agent_records(),
                                  hipMemcpyDeviceToHost, h->stream));
        return DW_OK;
    }
    // in front of a frame step: the field it computes, from its input planes
    int before(double L) {
        return temp ? launch_tile_temp(h, true, L, sh, h->frame_temp.get() + done % cap * sh.records()) : DW_OK;
    }
    // behind it: the cover of the state it left (and the agents on it); the ring goes down when it is full or the last
    // frame is in
    int after() {
        if (cover)
            if (int rc = launch_tile_cover(h, sh, h->cur, h->frame_cover.get() + done % cap * sh.records())) return rc;
        if (agents) {
            hipLaunchKernelGGL(frame_agents_pw, dim3((unsigned)((agent_records() + 255) / 256)), dim3(256), 0, h->stream, h->idx.get(),
                               h->st.get(), sh.listed ? h->frame_sel.get() : nullptr, sh.S, h->prm.n_agents,
                               h->frame_agents.get() + done % cap * agent_records());
            HIPCHK(hipGetLastError());
        }
        ++done;
        if (done % cap != 0 && done != total) return DW_OK;
        const size_t k = (done - 1) % cap + 1;
        return download(done - k, k);
    }
};

// f(MODE, PACK) for the strip layout of the fused kernels: packed worlds in rotating 256-column strips, the others by
// the plan's mode
template <class F>
static auto with_fused_layout(const StepPlan& pl, F&& f) {
    if (pl.packed) return f(int_c<kFusedRot>{}, std::true_type{});
    return with_int<kFusedRot, kFusedRing, kFusedOvl>(pl.fused_mode, [&](auto MODE) { return f(MODE, std::false_type{}); });
}

// Two steps (luminosities L1 then L2) in one launch on wide grids, no agent update in between.  The buffer
// that held the input now holds the state TWO steps back, so the retained "previous state" is not valid
// afterwards; dw_step_n always ends with an ordinary single step.
// `trace` (dw_step_n_trace, plans with trace_pairs): the TRACE kernels, which add the reductions of both steps into rows
// trace[0 .. B) and trace[B .. 2B).
static int launch_forward_fused2(dw_handle* h, double L1, double L2, unsigned int* pstats = nullptr,
                                 float thr_hi = 0.f, StatsDev* trace = nullptr) {
    const dw_params& p = h->prm;
    const StepPlan& pl = h->plan;
    const bool exact = p.precision == DW_PRECISION_EXACT;
    PhysF32 P1, P2;
    if (exact) derive_f32_pair(p, L1, L2, &P1, &P2);
    else { P1 = derive_f32(p, L1); P2 = derive_f32(p, L2); }
    const StepOut o = step_out(h);                              // (the pair's constants: P1, P2; no reductions)
    const FusedGeom& g = pl.fgeom;
    const dim3 grid((unsigned)g.chunk * 8u);
    const plane_t *inL = h->L16[h->cur].get(), *inD = h->D16[h->cur].get();
    auto exact_args = [&] {
        return FusedExactArgs{inL, inD, o.L, o.D, g, P1, lum_part(P2), o.zero_me, o.zero_n, pstats, thr_hi, make_f64(p, L1), L1, L2};
    };
    if (trace && exact) {
        const TraceExactArgs A{exact_args(), trace, h->sw.force_rescan ? 1 : 0};
        with_int<kFusedRot, kFusedOvl>(pl.fused_mode, [&](auto MODE) {
            with_bool(pl.sym_albedo, [&](auto SYM) {
                hipLaunchKernelGGL((trace_pair_exact<MODE, SYM>), grid, dim3(256), 0, h->stream, A);
            });
        });
    } else if (trace) {
        with_int<kFusedRot, kFusedOvl>(pl.fused_mode, [&](auto MODE) {
            hipLaunchKernelGGL((trace_pair_fast<MODE>), grid, dim3(256), 0, h->stream, inL, inD, o.L, o.D, g, P1, P2, o.zero_me,
                               o.zero_n, trace);
        });
    } else if (pl.seam_strips && !pstats && !exact) {
        const FusedGeom &gs = pl.seam_geom, &gl = pl.left_geom;
        const auto seam = pl.row_landing ? step_stream_fused2_land_seam_pw : step_stream_fused2_seam_pw;
        const auto left = pl.row_landing ? step_stream_fused2_land_left_pw : step_stream_fused2_left_pw;
        hipLaunchKernelGGL(seam, dim3((unsigned)gs.chunk * 8u), dim3(256), 0, h->stream, inL, inD, o.L, o.D, gs, P1, P2, o.zero_me,
                           o.zero_n);
        if (gl.nstrips)
            hipLaunchKernelGGL(left, dim3((unsigned)gl.chunk * 8u), dim3(256), 0, h->stream, inL, inD, o.L, o.D, gl, P1, P2,
                               o.zero_me, 0);
    } else if (pl.fmt_planes && !pstats && !exact) {
        hipLaunchKernelGGL((step_stream_fused2_fmt_pw<kFusedOvl>), grid, dim3(256), 0, h->stream, inL, inD, o.L, o.D, g, P1, P2,
                           o.zero_me, o.zero_n);
    } else if (exact) {
        const FusedExactArgs A = exact_args();
        with_bool(pstats != nullptr, [&](auto STATS) {
            with_fused_layout(pl, [&](auto MODE, auto PACK) {
                with_bool(pl.sym_albedo, [&](auto SYM) {
                    hipLaunchKernelGGL((step_stream_fused2_exact<MODE, PACK, STATS, SYM>), grid, dim3(256), 0, h->stream, A);
                });
            });
        });
    } else {
        with_bool(pstats != nullptr, [&](auto STATS) {
            with_fused_layout(pl, [&](auto MODE, auto PACK) {
                hipLaunchKernelGGL((step_stream_fused2<MODE, PACK, STATS>), grid, dim3(256), 0, h->stream, inL, inD, o.L, o.D, g,
                                   P1, P2, o.zero_me, o.zero_n, pstats, thr_hi);
            });
        });
    }
    HIPCHK(hipGetLastError());
    step_done(h, L2, false);      // the kernel cleared the old reductions; the (untouched, zero) other buffer is "current"
    return DW_OK;
}

static int launch_agents(dw_handle* h, const int* d_action, int act_b, int act_n, bool standalone = false,
                         double* d_reward = nullptr, unsigned char* d_done = nullptr, unsigned char* d_ok = nullptr) {
    const dw_params& p = h->prm;
    if (p.n_agents == 0) return DW_OK;
    NEED(h->have_state, DW_ESTATE, "no state uploaded");
    NEED(h->have_agents, DW_ESTATE, "no agents uploaded (call dw_upload_agents or dw_init_random)");
    NEED(p.collision_mode == 0 || standalone, DW_EINVAL,
         "collision_mode=1: call dw_update_agents, apply the collision pass (it consumes the caller's RNG) to the "
         "downloaded agent states, upload them, then dw_step without actions");
    const int blocks = (p.batch + 63) / 64;
    // grazing on the current state, in its own format (an un-quantised one included)
    with_planes(h, h->unq == OWN_CUR, h->cur, [&](auto* L, auto* D) {
        using T = elem_t<decltype(L)>;
        hipLaunchKernelGGL(agents_update<T>, dim3(blocks), dim3(64), 0, h->stream, L, D, h->idx.get(), h->st.get(), d_action,
                           act_b, act_n, p.batch, p.n_agents, p.height, p.width, p.agent_gamma,
                           p.collision_mode == 0 ? 1 : 0, d_reward, d_done, d_ok);
    });
    HIPCHK(hipGetLastError());
    return DW_OK;
}

static int stage_host_actions(dw_handle* h, const int32_t* action, int b, int n) {
    const dw_params& p = h->prm;
    NEED(b >= 0 && n >= 0 && b <= p.batch && n <= p.n_agents, DW_EINVAL,
         "action block %dx%d exceeds (B,N)=(%d,%d)", b, n, p.batch, p.n_agents);
    if ((size_t)b * n)
        HIPCHK(hipMemcpyAsync(h->action_tmp.get(), action, sizeof(int) * (size_t)b * n, hipMemcpyHostToDevice,
                              h->stream));
    return DW_OK;
}

// ------------------------------------------------------------------------------------------------
// a new state
// ------------------------------------------------------------------------------------------------
static int clear_stats(dw_handle* h) {
    for (int i = 0; i < 2; ++i) HIPCHK(hipMemsetAsync(h->stats2[i].get(), 0, h->stats_bytes, h->stream));
    return DW_OK;
}

// An upload or a draw has queued a new current state: quantised in the `cur` planes (OWN_NONE) or un-quantised in the
// buffers of `kind` (OWN_CUR).  There is no step pair any more, and no snapshot either (a snapshot's previous state may
// have lived in the un-quantised buffers).
static void state_arrived(dw_handle* h, UnqOwner unq, UnqKind kind = UNQ_F64) {
    if (unq == OWN_CUR) h->unq_kind = kind;
    h->unq = unq;
    h->have_state = true;
    h->stepped = false;
    for (auto& sn : h->snap) sn.valid = false;
}

// dw_init_random[_quantised]: the synthetic initial state drawn into the planes L, D, and the agents.  The draw reduces
// its own values into the per-world statistics (no second pass over the planes).
template <class T>
static auto init_random_into(dw_handle* h, uint64_t seed, T* L, T* D) {
    const dw_params& p = h->prm;
    if (int crc = clear_stats(h)) return crc;
    const int ncell = p.height * p.width;
    for_world_slices(p.batch, [&](int b0, int nb) {              // (the draw is keyed by the GLOBAL world id: offset + b0 + b)
        const dim3 g((unsigned)((ncell + kInitChunk - 1) / kInitChunk), (unsigned)nb);
        const size_t w = (size_t)b0 * ncell;
        hipLaunchKernelGGL((init_random_cells<T>), g, dim3(256), 0, h->stream, L + w, D + w, ncell,
                           (long long)p.world_offset + b0, (unsigned long long)seed, (float)p.light_proportion,
                           (float)p.dark_proportion, (float)p.initial_al, (float)p.initial_ad, h->stats2[h->sp].get() + b0);
    });
    HIPCHK(hipGetLastError());
    if (p.n_agents) {
        const int bn = p.batch * p.n_agents;
        hipLaunchKernelGGL(init_random_agents, dim3((bn + 255) / 256), dim3(256), 0, h->stream, h->idx.get(), h->st.get(),
                           p.batch, p.n_agents, p.height, p.width, (long long)p.world_offset,
                           (unsigned long long)seed);
        HIPCHK(hipGetLastError());
    }
    h->have_agents = true;
    return (int)DW_OK;                          // (statistics: reduced by the draw itself)
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

const char* dw_last_error(void) { return g_err; }
int dw_abi_version(void) { return DW_ABI_VERSION; }

int dw_pinned_alloc(size_t bytes, void** out) {
    NEED(out && bytes > 0, DW_EINVAL, "null argument");
    int ndev = 0;
    NEED(hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0, DW_ENODEVICE, "no HIP device");
    HIPCHK(hipHostMalloc(out, bytes, hipHostMallocDefault));
    return DW_OK;
}
int dw_pinned_free(void* p) {
    if (p) HIPCHK(hipHostFree(p));
    return DW_OK;
}

#ifndef DW_BUILD_ID
#define DW_BUILD_ID "unknown"
#endif
// the marker makes the id findable in the file without loading it (therldaisyworld_amd/build.py)
static const char kBuildId[] = "DW_BUILD_ID=" DW_BUILD_ID;
const char* dw_build_id(void) { return kBuildId + 12; }

int dw_default_params(dw_params* p, int32_t batch, int32_t height, int32_t width, int32_t n_agents) {
    NEED(p, DW_EINVAL, "null params");
    std::memset(p, 0, sizeof(*p));
    p->abi_version = DW_ABI_VERSION;
    p->batch = batch; p->height = height; p->width = width; p->n_agents = n_agents;
    p->device = 0; p->precision = DW_PRECISION_EXACT; p->obs_mask = 0x0BA; p->collision_mode = 0;
    p->world_offset = 0;
    p->p = 1.0; p->g = 0.003265; p->S = 1000.0; p->sigma = 5.67e-8; p->gamma = 0.25;
    p->q = 0.2 * p->S / p->sigma; p->q2 = p->q / 8.0; p->dt = 1.0;
    p->albedo_bare = 0.5; p->albedo_light = 0.75; p->albedo_dark = 0.25; p->temp_optimal = 295.5;
    p->agent_gamma = 0.05; p->food_chain_penalty = 0.5;
    p->initial_al = 0.2; p->initial_ad = 0.2; p->light_proportion = 0.33; p->dark_proportion = 0.33;
    return DW_OK;
}

static int check_params(const dw_params* p) {
    NEED(p, DW_EINVAL, "null params");
    NEED(p->abi_version == DW_ABI_VERSION, DW_EINVAL, "ABI version %d != %d", p->abi_version, DW_ABI_VERSION);
    NEED(p->batch >= 1 && p->height >= 3 && p->width >= 3, DW_EINVAL,
         "need batch>=1 and grid >= 3x3 (got B=%d H=%d W=%d)", p->batch, p->height, p->width);
    NEED(p->height <= 65535 && p->width <= 65532, DW_EINVAL, "grid dimension too large");
    // cell indices inside one world are int32 in the host code and in every kernel; everything above a world - its base,
    // the per-world tables and records - is 64-bit.  The batch has no cap of its own: the kernels that take the world from
    // blockIdx.y are launched in slices of 65 535 worlds (for_world_slices), every other kernel numbers strips, tiles or
    // worlds in blockIdx.x (tests/test_gpu_large_offsets.py: 70 000 and 1 943 000 worlds, 2^32 cells)
    NEED((long long)p->height * p->width <= 0x7fffffffLL, DW_EINVAL,
         "a world of %dx%d cells exceeds the 2^31-1 cells per world the kernels index", p->height, p->width);
    NEED(p->n_agents >= 0, DW_EINVAL, "n_agents < 0");
    NEED(p->precision >= 0 && p->precision <= 2, DW_EINVAL, "bad precision %d", p->precision);
    NEED(p->precision == DW_PRECISION_F64 || p->g >= 0.0, DW_EINVAL,
         "g < 0 (a growth curve opening upwards) is evaluated by DW_PRECISION_F64 only");
    NEED((double)p->batch * p->height * p->width < 9.0e18, DW_EINVAL, "too many cells");
    return DW_OK;
}

int dw_create(const dw_params* p, dw_handle** out) {
    NEED(out, DW_EINVAL, "null out");
    *out = nullptr;
    int rc = check_params(p);
    if (rc) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(DW_ENODEVICE, "no HIP device available (this library has no CPU fallback)");
    NEED(p->device >= 0 && p->device < ndev, DW_ENODEVICE, "device %d out of range (%d devices)", p->device, ndev);
    HIPCHK(hipSetDevice(p->device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, p->device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(DW_ENODEVICE, "device %d is %s; this library is built for gfx950 only", p->device,
                    prop.gcnArchName);
    // a handle that is not complete is destroyed on the way out (dw_destroy; its buffers by their owners)
    std::unique_ptr<dw_handle, int (*)(dw_handle*)> h(new (std::nothrow) dw_handle(), dw_destroy);
    NEED(h, DW_ENOMEM, "host allocation failed");
    h->prm = *p;
    h->cells = (size_t)p->batch * p->height * p->width;
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->own_stream = true;
    const size_t bn = (size_t)p->batch * (p->n_agents > 0 ? p->n_agents : 1);
    const size_t pb = sizeof(plane_t) * h->cells;
    // [(B+1) StatsDev][(kNumQueues+1)*16 uint queue counters]
    h->stats_bytes = sizeof(StatsDev) * (p->batch + 1) + sizeof(unsigned int) * (kNumQueues + 1) * 16;
    if (int rc = alloc_group(h.get(), "the handle's state",
                             {{h->L16[0], pb}, {h->D16[0], pb}, {h->L16[1], pb}, {h->D16[1], pb},
                              {h->idx, sizeof(int) * bn * 2}, {h->st, sizeof(double) * bn}, {h->action, sizeof(int) * bn},
                              {h->action_tmp, sizeof(int) * bn}, {h->reward_d, sizeof(double) * bn}, {h->done_d, bn},
                              {h->agents_done_at, sizeof(int) * bn}, {h->done_at, sizeof(int) * p->batch},
                              {h->n_alive, sizeof(int)}, {h->stats2[0], h->stats_bytes}, {h->stats2[1], h->stats_bytes},
                              {h->side_stats, sizeof(StatsDev) * (p->batch + 1)}}))
        return rc;
    for (int i = 0; i < 2; ++i) HIPCHK(hipMemsetAsync(h->stats2[i].get(), 0, h->stats_bytes, h->stream));
    h->sw = read_switches();                                    // the environment is read here and nowhere else
    h->plan = plan_steps(*p, h->sw);
    if (int rc = ensure_fixq(h.get(), h->plan)) return rc;
    HIPCHK(hipMemsetAsync(h->action.get(), 0, sizeof(int) * bn, h->stream));
    HIPCHK(hipMemsetAsync(h->done_at.get(), 0, sizeof(int) * p->batch, h->stream));
    HIPCHK(hipMemsetAsync(h->agents_done_at.get(), 0, sizeof(int) * bn, h->stream));
    HIPCHK(hipMemsetAsync(h->n_alive.get(), 0, sizeof(int), h->stream));
    HIPCHK(hipEventCreate(&h->ev0));
    HIPCHK(hipEventCreate(&h->ev1));
    HIPCHK(hipEventCreate(&h->evf0));
    HIPCHK(hipEventCreate(&h->evf1));
    h->created = true;
    *out = h.release();
    return DW_OK;
}

int dw_destroy(dw_handle* h) {
    if (!h) return DW_OK;
    (void)hipSetDevice(h->prm.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->evf0) (void)hipEventDestroy(h->evf0);
    if (h->evf1) (void)hipEventDestroy(h->evf1);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;                                                   // the owners give the buffers back
    return DW_OK;
}

int dw_set_params(dw_handle* h, const dw_params* p) {
    NEED(h, DW_EINVAL, "null handle");
    int rc = check_params(p);
    if (rc) return rc;
    const dw_params& o = h->prm;
    NEED(p->batch == o.batch && p->height == o.height && p->width == o.width && p->n_agents == o.n_agents &&
             p->device == o.device,
         DW_EINVAL, "dw_set_params cannot change shape or device; create a new handle");
    HIPCHK(hipSetDevice(p->device));
    const StepPlan plan = plan_steps(*p, h->sw);
    if ((rc = ensure_fixq(h, plan))) return rc;                 // a failure leaves the handle as it was
    h->prm = *p;
    h->plan = plan;
    return DW_OK;
}

int dw_get_params(const dw_handle* h, dw_params* out) {
    NEED(h && out, DW_EINVAL, "null argument");
    *out = h->prm;
    return DW_OK;
}

// ---- state in / out ---------------------------------------------------------------------------

// reductions of the current state, whatever its format (after uploads, so that dw_reduce is always valid)
static int refresh_stats(dw_handle* h) {
    const dw_params& p = h->prm;
    if (int rc = clear_stats(h)) return rc;
    const int n = p.height * p.width;
    auto reduce = [&](auto* L, auto* D) {
        for_world_slices(p.batch, [&](int b0, int nb) {
            const dim3 g((unsigned)((n + kInitChunk - 1) / kInitChunk), (unsigned)nb);
            const size_t w = (size_t)b0 * n;
            hipLaunchKernelGGL((stats_only<elem_t<decltype(L)>>), g, dim3(256), 0, h->stream, L + w, D + w, n,
                               h->stats2[h->sp].get() + b0);
        });
    };
    if (cur_quantised(h)) reduce(h->L16[h->cur].get(), h->D16[h->cur].get());
    else with_unq_planes(h, reduce);
    HIPCHK(hipGetLastError());
    return DW_OK;
}

int dw_upload_state_f64(dw_handle* h, const double* light, const double* dark) {
    NEED(h && light && dark, DW_EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->prm.device));
    if (int arc = ensure_f64(h)) return arc;
    HIPCHK(hipMemcpyAsync(h->L64.get(), light, sizeof(double) * h->cells, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->D64.get(), dark, sizeof(double) * h->cells, hipMemcpyHostToDevice, h->stream));
    state_arrived(h, OWN_CUR, UNQ_F64);
    int rc = refresh_stats(h);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));   // host buffers may be reused by the caller
    return DW_OK;
}

int dw_upload_state_f32(dw_handle* h, const float* light, const float* dark, int quantised) {
    NEED(h && light && dark, DW_EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->prm.device));
    const unsigned blocks = (unsigned)((h->cells + 255) / 256);
    if (quantised) {
        // natural-unit floats staged in scratch, rounded to the per-mille integers of the canonical planes
        int rc = ensure_scratch(h, sizeof(float) * 2 * h->cells);
        if (rc) return rc;
        float* sL = reinterpret_cast<float*>(h->scratch.get());
        float* sD = sL + h->cells;
        HIPCHK(hipMemcpyAsync(sL, light, sizeof(float) * h->cells, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(sD, dark, sizeof(float) * h->cells, hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(f32nat_to_plane, dim3(blocks), dim3(256), 0, h->stream, sL, h->L16[h->cur].get(), h->cells);
        hipLaunchKernelGGL(f32nat_to_plane, dim3(blocks), dim3(256), 0, h->stream, sD, h->D16[h->cur].get(), h->cells);
        HIPCHK(hipGetLastError());
        state_arrived(h, OWN_NONE);
    } else {
        int rc = ensure_u32(h);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(h->U32L.get(), light, sizeof(float) * h->cells, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->U32D.get(), dark, sizeof(float) * h->cells, hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(f32nat_to_permille, dim3(blocks), dim3(256), 0, h->stream, h->U32L.get(), h->U32L.get(), h->cells);
        hipLaunchKernelGGL(f32nat_to_permille, dim3(blocks), dim3(256), 0, h->stream, h->U32D.get(), h->U32D.get(), h->cells);
        HIPCHK(hipGetLastError());
        state_arrived(h, OWN_CUR, UNQ_F32);
    }
    int rc = refresh_stats(h);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return DW_OK;
}

int dw_upload_agents(dw_handle* h, const int32_t* indices, const double* states) {
    NEED(h, DW_EINVAL, "null handle");
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    const size_t bn = (size_t)p.batch * p.n_agents;
    if (bn) {
        NEED(indices && states, DW_EINVAL, "null argument");
        for (size_t i = 0; i < bn; ++i) {
            NEED(indices[2 * i] >= 0 && indices[2 * i] < p.height && indices[2 * i + 1] >= 0 &&
                     indices[2 * i + 1] < p.width,
                 DW_EINVAL, "agent %zu position (%d,%d) outside the %dx%d grid", i, indices[2 * i],
                 indices[2 * i + 1], p.height, p.width);
        }
        HIPCHK(hipMemcpyAsync(h->idx.get(), indices, sizeof(int) * bn * 2, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->st.get(), states, sizeof(double) * bn, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    h->have_agents = true;
    return DW_OK;
}

int dw_download_agents(dw_handle* h, int32_t* indices, double* states) {
    NEED(h, DW_EINVAL, "null handle");
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    const size_t bn = (size_t)p.batch * p.n_agents;
    if (bn) {
        NEED(h->have_agents, DW_ESTATE, "no agents");
        if (indices) HIPCHK(hipMemcpyAsync(indices, h->idx.get(), sizeof(int) * bn * 2, hipMemcpyDeviceToHost, h->stream));
        if (states) HIPCHK(hipMemcpyAsync(states, h->st.get(), sizeof(double) * bn, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return DW_OK;
}

int dw_init_random(dw_handle* h, uint64_t seed) {
    NEED(h, DW_EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->prm.device));
    if (int rc = ensure_u32(h)) return rc;      // the synthetic initial state is un-quantised like the reference's
    if (int rc = init_random_into(h, seed, h->U32L.get(), h->U32D.get())) return rc;
    state_arrived(h, OWN_CUR, UNQ_F32);
    return DW_OK;
}

int dw_init_random_quantised(dw_handle* h, uint64_t seed) {
    NEED(h, DW_EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->prm.device));
    if (int rc = init_random_into(h, seed, h->L16[h->cur].get(), h->D16[h->cur].get())) return rc;
    state_arrived(h, OWN_NONE);
    release_unquantised(h);
    return DW_OK;
}

int dw_download_planes(dw_handle* h, int which, double* light, double* dark) {
    NEED(h, DW_EINVAL, "null handle");
    NEED(h->have_state, DW_ESTATE, "no state");
    HIPCHK(hipSetDevice(h->prm.device));
    NEED(which == DW_STATE_CURRENT || which == DW_STATE_PREVIOUS, DW_EINVAL, "bad state selector");
    NEED(which == DW_STATE_CURRENT || h->stepped, DW_ESTATE, "no previous state before the first step");
    const int buf = which == DW_STATE_CURRENT ? h->cur : 1 - h->cur;
    const bool unq = (which == DW_STATE_CURRENT && h->unq == OWN_CUR) || (which == DW_STATE_PREVIOUS && h->unq == OWN_PREV);
    const size_t bytes = sizeof(double) * h->cells;
    if (unq && h->unq_kind == UNQ_F64) {
        if (light) HIPCHK(hipMemcpyAsync(light, h->L64.get(), bytes, hipMemcpyDeviceToHost, h->stream));
        if (dark) HIPCHK(hipMemcpyAsync(dark, h->D64.get(), bytes, hipMemcpyDeviceToHost, h->stream));
    } else {
        int rc = ensure_scratch(h, bytes);
        if (rc) return rc;
        const unsigned blocks = (unsigned)((h->cells + 255) / 256);
        for (int pl = 0; pl < 2; ++pl) {
            double* dst = pl == 0 ? light : dark;
            if (!dst) continue;
            if (unq)
                hipLaunchKernelGGL((plane_to_f64<float>), dim3(blocks), dim3(256), 0, h->stream,
                                   pl == 0 ? h->U32L.get() : h->U32D.get(), h->scratch.get(), h->cells);
            else
                hipLaunchKernelGGL((plane_to_f64<plane_t>), dim3(blocks), dim3(256), 0, h->stream,
                                   pl == 0 ? h->L16[buf].get() : h->D16[buf].get(), h->scratch.get(), h->cells);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(dst, h->scratch.get(), bytes, hipMemcpyDeviceToHost, h->stream));
        }
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return DW_OK;
}

// materialise into device scratch: grid7 and/or caches
static int run_materialise(dw_handle* h, double L, double* d_grid7, double* d_temps, double* d_betas,
                           double* d_growth, double* d_teff) {
    const dw_params& p = h->prm;
    const PhysF64 P = make_f64(p, h->stepped && !h->L_per_world ? h->L_last : L);   // (per-world: dw_download_caches' own L)
    const plane_t* cL = h->L16[h->cur].get();            // read by the POST variants only
    const plane_t* cD = h->D16[h->cur].get();
    with_derived_from(h, [&](auto* pL, auto* pD, auto POST) {
        launch_materialise<elem_t<decltype(pL)>, POST>(h, pL, pD, cL, cD, P, d_grid7, d_temps, d_betas, d_growth, d_teff);
    });
    HIPCHK(hipGetLastError());
    if (h->stepped && d_grid7 && p.n_agents && h->have_agents) {
        hipLaunchKernelGGL(agents_stamp, dim3((p.batch + 63) / 64), dim3(64), 0, h->stream, d_grid7, h->idx.get(),
                           h->st.get(), p.batch, p.n_agents, p.height, p.width);
        HIPCHK(hipGetLastError());
    }
    return DW_OK;
}

int dw_download_grid(dw_handle* h, double L_init, double* grid7) {
    NEED(h && grid7, DW_EINVAL, "null argument");
    NEED(h->have_state, DW_ESTATE, "no state");
    NEED_SHARED_L(h, "dw_download_grid");
    HIPCHK(hipSetDevice(h->prm.device));
    const size_t bytes = sizeof(double) * 7 * h->cells;
    int rc = ensure_scratch(h, bytes);
    if (rc) return rc;
    rc = run_materialise(h, L_init, h->scratch.get(), nullptr, nullptr, nullptr, nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(grid7, h->scratch.get(), bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return DW_OK;
}

int dw_download_caches(dw_handle* h, double L, double* temps, double* betas, double* growth,
                       double* temp_effective) {
    NEED(h, DW_EINVAL, "null handle");
    NEED(h->have_state, DW_ESTATE, "no state");
    NEED_SHARED_CONSTANTS(h, "dw_download_caches");
    HIPCHK(hipSetDevice(h->prm.device));
    const size_t n = h->cells;
    int rc = ensure_scratch(h, sizeof(double) * 9 * n);
    if (rc) return rc;
    double* d_t = h->scratch.get();
    double* d_b = d_t + 3 * n;
    double* d_g = d_b + 3 * n;
    double* d_e = d_g + 2 * n;
    rc = run_materialise(h, L, nullptr, temps ? d_t : nullptr, betas ? d_b : nullptr, growth ? d_g : nullptr,
                         temp_effective ? d_e : nullptr);
    if (rc) return rc;
    if (temps) HIPCHK(hipMemcpyAsync(temps, d_t, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, h->stream));
    if (betas) HIPCHK(hipMemcpyAsync(betas, d_b, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, h->stream));
    if (growth) HIPCHK(hipMemcpyAsync(growth, d_g, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, h->stream));
    if (temp_effective) HIPCHK(hipMemcpyAsync(temp_effective, d_e, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return DW_OK;
}

int dw_reduce_temperature(dw_handle* h, double L, dw_temp_stats* per_world) {
    NEED(h && per_world, DW_EINVAL, "null argument");
    NEED(h->have_state, DW_ESTATE, "no state");
    NEED_SHARED_CONSTANTS(h, "dw_reduce_temperature");
    static_assert(sizeof(dw_temp_stats) == sizeof(TempStatsDev), "temperature record layout");
    HIPCHK(hipSetDevice(h->prm.device));
    const size_t bytes = sizeof(TempStatsDev) * (size_t)h->prm.batch;
    if (int rc = alloc_group(h, "the temperature reduction", {{h->temp_part, temp_part_bytes(h)}, {h->temp_d, bytes}})) return rc;
    // (the luminosity: run_materialise's rule - the caches' own)
    if (int rc = launch_temp_moments(h, false, h->stepped && !h->L_per_world ? h->L_last : L, nullptr, h->temp_d.get())) return rc;
    HIPCHK(hipMemcpyAsync(per_world, h->temp_d.get(), bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return DW_OK;
}

// ---- the hot path -----------------------------------------------------------------------------

int dw_update_agents(dw_handle* h, const int32_t* action, int32_t action_b, int32_t action_n) {
    NEED(h && action, DW_EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->prm.device));
    int rc = stage_host_actions(h, action, action_b, action_n);
    if (rc) return rc;
    return launch_agents(h, h->action_tmp.get(), action_b, action_n, true);
}

int dw_step(dw_handle* h, const int32_t* action, int32_t action_b, int32_t action_n, double L) {
    NEED(h, DW_EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->prm.device));
    if (action) {
        int rc = stage_host_actions(h, action, action_b, action_n);
        if (rc) return rc;
        rc = launch_agents(h, h->action_tmp.get(), action_b, action_n);
        if (rc) return rc;
    }
    return launch_forward(h, L);
}

int dw_step_device_actions(dw_handle* h, double L) {
    NEED(h, DW_EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->prm.device));
    int rc = launch_agents(h, h->action.get(), h->prm.batch, h->prm.n_agents);
    if (rc) return rc;
    return launch_forward(h, L);
}

int dw_upload_actions(dw_handle* h, const int32_t* action) {
    NEED(h && action, DW_EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->prm.device));
    const size_t bn = (size_t)h->prm.batch * h->prm.n_agents;
    if (bn) {
        HIPCHK(hipMemcpyAsync(h->action.get(), action, sizeof(int) * bn, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return DW_OK;
}

int dw_download_actions(dw_handle* h, int32_t* action) {
    NEED(h && action, DW_EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->prm.device));
    const size_t bn = (size_t)h->prm.batch * h->prm.n_agents;
    if (bn) HIPCHK(hipMemcpyAsync(action, h->action.get(), sizeof(int) * bn, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return DW_OK;
}

int dw_step_n(dw_handle* h, int32_t nsteps, double* L_io, double dL, double min_L, double max_L,
              int use_device_actions) {
    NEED(h && L_io, DW_EINVAL, "null argument");
    NEED(nsteps >= 0, DW_EINVAL, "nsteps < 0");
    HIPCHK(hipSetDevice(h->prm.device));
    double L = *L_io;
    auto advance = [&]() { L += dL; L = L > max_L ? max_L : L; L = L < min_L ? min_L : L; };   // ref update_L :471-473
    int s0 = 0;
    h->fused_launches = 0;
    if (!use_device_actions && nsteps >= 1 && h->have_state && !cur_quantised(h)) {
        int rc = launch_forward(h, L);          // the first step reads the un-quantised state in its own format
        if (rc) return rc;
        advance();
        s0 = 1;
    }
    // Small worlds: keep the whole run of steps on the chip (worlds in LDS, one launch per 4096 steps) -
    // unless the ensemble is big enough to fill the GPU with wave-strips, where the packed fused kernel is
    // 1.5-1.8x faster (measured crossover between 2 M and 16 M cells: tools/kbench.py 512 64 / 4096 64).
    const bool big_packed = h->plan.allow_fuse && h->plan.packed && h->cells >= ((size_t)1 << 23);
    // (the episode kernels stage the agents of a world with it: a handle whose agents were never uploaded takes the step
    // kernels below, which - like dw_step without actions - do not look at them)
    if (!use_device_actions && nsteps - s0 > 1 && h->have_state && h->prm.height * h->prm.width <= 4096 && !big_packed &&
        (h->prm.n_agents == 0 || h->have_agents) && episode_kernel_applies(h)) {
        std::vector<double> Ls;
        while (s0 < nsteps) {
            const int k = nsteps - s0 < 4096 ? nsteps - s0 : 4096;
            Ls.resize(k);
            for (int i = 0; i < k; ++i) { Ls[i] = L; advance(); }
            int rc = run_episode_impl(h, k, Ls.data(), kPolicySkipAgents, nullptr, nullptr, 5, nullptr, nullptr);
            if (rc) return rc;
            s0 += k;
        }
        *L_io = L;
        return DW_OK;
    }
    if (!use_device_actions && h->plan.allow_fuse && h->have_state && nsteps - s0 >= 3) {
        // wide grids: pairs of steps share one HBM round trip; the last one or two steps are ordinary launches
        // so that the retained previous state is the true predecessor.  HIP events around the run of fused
        // launches feed dw_last_step_n_timing (the dominant kernel's duration, measured on its own stream).
        drop_unquantised_previous(h);
        HIPCHK(hipEventRecord(h->evf0, h->stream));
        int launched = 0;
        while (nsteps - s0 >= 3) {
            const double L1 = L;
            advance();
            const double L2 = L;
            advance();
            int rc = launch_forward_fused2(h, L1, L2);
            if (rc) return rc;                  // fused_launches stays 0: no timing of a run that was cut short
            s0 += 2;
            launched += 1;
        }
        HIPCHK(hipEventRecord(h->evf1, h->stream));
        h->fused_launches = launched;           // valid only now that evf1 is recorded
    }
    for (int s = s0; s < nsteps; ++s) {
        int rc;
        if (use_device_actions) {
            rc = launch_agents(h, h->action.get(), h->prm.batch, h->prm.n_agents);
            if (rc) return rc;
        }
        rc = launch_forward(h, L);
        if (rc) return rc;
        advance();
    }
    *L_io = L;
    return DW_OK;
}

// ---- the step series: dw_step_n_trace and its temperature, per-world and ensemble forms -----------------------------
// dw_step_n_trace_ensemble takes step pairs (trace_pair_fast_pw) on the plans dw_step_n_trace does, in the float32-only
// mode; the exact pair kernel does not keep its row loop with constants from a table (dw_step_fused_pw.hpp)
static bool ensemble_pairs(const dw_handle* h) { return h->plan.trace_pairs && h->prm.precision == DW_PRECISION_FAST; }

// What the per-world calls check before anything is launched or allocated: their schedule, and their worlds - a world's
// params as `rows` derives from them, the handle's with the world's members (check_params refuses among those only g:
// g < 0 in the float32 precisions)
static int check_per_world(const WorldRows& rows, const dw_world_params* worlds, const double* L_schedule, size_t nsteps, size_t B) {
    for (size_t i = 0; i < nsteps * B; ++i)
        NEED(std::isfinite(L_schedule[i]) && L_schedule[i] >= 0.0, DW_EINVAL,
             "L_schedule[step %zu][world %zu] = %g: a luminosity is finite and not negative", i / B, i % B, L_schedule[i]);
    for (size_t b = 0; worlds && b < B; ++b) {
        if (check_params(&rows.params(b)) != DW_OK) {
            char why[sizeof(g_err)];
            snprintf(why, sizeof(why), "%s", g_err);
            return fail(DW_EINVAL, "worlds[%zu].g = %g: %s", b, worlds[b].g, why);
        }
    }
    return DW_OK;
}

// The device side of the per-world table (PwLayout): the handle's buffer and its page-locked image, and the event after
// which the image may be written again.
struct PwTable {
    dw_handle* h;
    const PwLayout lay;
    hipEvent_t uploaded = nullptr;
    bool in_flight = false;
    PwTable(dw_handle* h_, const PwLayout& lay_) : h(h_), lay(lay_) {}
    PwTable(const PwTable&) = delete;
    ~PwTable() { if (uploaded) (void)hipEventDestroy(uploaded); }
    unsigned char* img() const { return h->pw_pinned.get(); }
    unsigned char* dev() const { return h->pw_tab.get(); }
    GroupItem<DeviceMem> item() const { return {h->pw_tab, lay.bytes}; }
    // `group`: item() and what the call uses with the table, all or nothing; then the image
    int alloc(const char* what, std::initializer_list<GroupItem<DeviceMem>> group) {
        if (int rc = alloc_group(h, what, group)) return rc;
        if (int rc = reserve(h->pw_pinned, "the page-locked image of the per-world constants", lay.bytes)) {
            h->pw_tab.reset();
            return rc;
        }
        HIPCHK(hipEventCreateWithFlags(&uploaded, hipEventDisableTiming));
        return DW_OK;
    }
    // chunk c of a schedule: derived in float64 into the image once it is free; the rows in use of each part go up in one
    // copy each (`first_bound`: row 0 of the first chunk is step 0, from an un-quantised state in the exact mode)
    int next_chunk(const SeriesSchedule& q, size_t c, const double* Ls, WorldRows& worlds, bool first_bound = false) {
        if (in_flight) HIPCHK(hipEventSynchronize(uploaded));
        fill_chunk(q, c, Ls, worlds, lay, img());
        if (first_bound) worlds.first_bound(Ls, lay.p32(img(), 0), h->unq_kind == UNQ_F64, h->sw.first_slack, lay.fb(img()));
        auto part = [&](size_t off, size_t bytes) { return hipMemcpyAsync(dev() + off, img() + off, bytes, hipMemcpyHostToDevice, h->stream); };
        const size_t singles = q.chunks[c].singles, pairs = q.chunks[c].pairs;
        if (singles) {
            HIPCHK(part(0, sizeof(PhysF32) * singles * lay.B));
            HIPCHK(part(lay.o64, sizeof(PhysF64) * singles * lay.B));
        }
        if (first_bound) HIPCHK(part(lay.ofb, sizeof(FirstStepBound) * lay.B));
        if (pairs) HIPCHK(part(lay.opair, sizeof(PairPw) * pairs * lay.B));
        HIPCHK(hipEventRecord(uploaded, h->stream));
        in_flight = true;
        return DW_OK;
    }
};

// One series call in flight.  The constants of its steps have two sources: the handle's own at the shared luminosity
// Ls[t], or (`table`) rows of the per-world table derived from Ls[t][B].
struct SeriesRun {
    dw_handle* h;
    const SeriesSchedule& q;
    const double* Ls;
    dw_world_stats* trace;            // what the caller wants of each series (either may be null)
    dw_temp_stats* temps;
    PwTable* table;
    bool sym, constants;              // (table) what launch_forward_pw takes besides its rows
    size_t B, row_bytes, trow_bytes;
    bool first_pair = true;
    FrameRun* frames = nullptr;       // dw_step_n_frames: the tile maps around the steps the schedule marks
    // the reductions of every step go to a row of trace_d: a series is wanted, or pair kernels add theirs there
    bool keep_rows() const { return trace || q.even; }

    int alloc() {
        const GroupItem<DeviceMem> tr{h->trace_d, keep_rows() ? q.rows * row_bytes : 0}, part{h->temp_part, temp_part_bytes(h)},
            td{h->temp_d, q.rows * trow_bytes};
        if (frames)
            return alloc_group(h, "the trace buffer and the frame buffers",
                               {tr, {h->frame_sel, frames->sh.sel_bytes()}, {h->frame_cover, frames->cover_bytes()},
                                {h->frame_temp, frames->temp_bytes()}, {h->tile_part, frames->sh.part_bytes()}});
        if (!table) return temps ? alloc_group(h, "the trace buffer and the temperature reduction", {tr, part, td})
                                 : alloc_group(h, "the trace buffer", {tr});
        if (temps) return table->alloc("the per-world constants, the trace buffer and the temperature reduction", {table->item(), tr, part, td});
        return keep_rows() ? table->alloc("the per-world constants and the trace buffer", {table->item(), tr})
                           : table->alloc("the per-world constants", {table->item()});
    }
    // step t, or the pair that starts there; the field a step computes is reduced from its input planes, in front of it
    int step(int t) {
        const size_t sr = (size_t)t % q.rows, tr = table ? q.row_of[(size_t)t] : 0;
        StatsDev* row = keep_rows() ? h->trace_d.get() + sr * B : nullptr;
        unsigned char* tab = table ? table->dev() : nullptr;
        if (q.is_pair[(size_t)t]) {
            if (first_pair) drop_unquantised_previous(h);
            first_pair = false;
            return table ? launch_forward_fused2_pw(h, table->lay.pair(tab, tr), row)
                         : launch_forward_fused2(h, Ls[t], Ls[t + 1], nullptr, 0.f, row);
        }
        const PhysF64* r64 = table ? table->lay.p64(tab, tr) : nullptr;
        if (temps)
            if (int rc = launch_temp_moments(h, true, table ? 0.0 : Ls[t], r64, h->temp_d.get() + sr * B)) return rc;
        const bool frame = frames && q.is_frame[(size_t)t];
        if (frame)
            if (int rc = frames->before(Ls[t])) return rc;
        if (int rc = table ? launch_forward_pw(h, table->lay.p32(tab, tr), r64, table->lay.fb(tab), sym, constants)
                           : launch_forward(h, Ls[t])) return rc;
        if (row) HIPCHK(hipMemcpyAsync(row, h->stats2[h->sp].get(), row_bytes, hipMemcpyDeviceToDevice, h->stream));
        return frame ? frames->after() : DW_OK;
    }
    int run(WorldRows* worlds) {
        const int nsteps = (int)q.is_pair.size();
        const bool first_bound = h->unq == OWN_CUR && h->plan.first_prec == 3;
        size_t c = 0;                                           // the table chunk that starts next
        for (int t = 0; t < nsteps; t += q.took(t)) {
            const size_t sr = (size_t)t % q.rows, left = (size_t)(nsteps - t), filled = sr + (size_t)q.took(t);
            if (table && t == (c ? q.chunks[c - 1].end : 0)) {
                if (int rc = table->next_chunk(q, c, Ls, *worlds, c == 0 && first_bound)) return rc;
                ++c;
            }
            if (q.even && sr == 0)                              // the pair kernels ADD their reductions into the rows
                HIPCHK(hipMemsetAsync(h->trace_d.get(), 0, (left < q.rows ? left : q.rows) * row_bytes, h->stream));
            if (int rc = step(t)) return rc;
            if (filled != q.rows && t + q.took(t) != nsteps) continue;
            const size_t r0 = ((size_t)t - sr) * B;             // the chunk of the series is full or the run is over
            if (temps) HIPCHK(hipMemcpyAsync(temps + r0, h->temp_d.get(), filled * trow_bytes, hipMemcpyDeviceToHost, h->stream));
            if (trace) HIPCHK(hipMemcpyAsync(trace + r0, h->trace_d.get(), filled * row_bytes, hipMemcpyDeviceToHost, h->stream));
        }
        return DW_OK;
    }
};

// The five dw_step_n_trace* calls after their null checks.  The per-world forms take L_schedule[nsteps][B], world b's rows
// from the handle's params with worlds[b]'s members when there are `worlds`; after PER_WORLD_CONSTANTS the handle remembers
// that the constants were per-world.  `always_even`, `may_pair`: plan_series.
enum SeriesForm { SHARED_L, PER_WORLD_L, PER_WORLD_CONSTANTS };
static int run_series(dw_handle* h, int32_t nsteps, const double* L_schedule, dw_world_stats* trace, dw_temp_stats* temps,
                      bool always_even, bool may_pair, SeriesForm form = SHARED_L, const dw_world_params* worlds = nullptr,
                      FrameRun* frames = nullptr) {
    const bool pw = form != SHARED_L;
    NEED(nsteps >= 0, DW_EINVAL, "nsteps < 0");
    if (nsteps == 0) return DW_OK;
    NEED(h->have_state, DW_ESTATE, "no state uploaded (call dw_upload_state_* or dw_init_random)");
    static_assert(sizeof(dw_world_stats) == sizeof(StatsDev), "stats layout");
    static_assert(sizeof(dw_temp_stats) == sizeof(TempStatsDev), "temperature record layout");
    const dw_params& p = h->prm;
    const size_t B = (size_t)p.batch;
    std::unique_ptr<WorldRows> rows(pw ? new WorldRows(p, worlds, B) : nullptr);
    if (int rc = pw ? check_per_world(*rows, worlds, L_schedule, (size_t)nsteps, B) : DW_OK) return rc;
    const bool sym = worlds ? worlds_symmetric(worlds, B) && !h->sw.no_sym : h->plan.sym_albedo;
    HIPCHK(hipSetDevice(p.device));
    const SeriesSchedule q = plan_series(SeriesSpec{nsteps, B, sizeof(StatsDev), sizeof(TempStatsDev), h->sw.trace_rows, always_even,
                                                    may_pair, cur_quantised(h), temps != nullptr, pw ? L_schedule : nullptr,
                                                    frames ? frames->stride : 0, frames && frames->temp});
    if (frames) frames->plan(q.nframes);
    std::unique_ptr<PwTable> table(pw ? new PwTable(h, PwLayout(B, q.trows, q.prows)) : nullptr);
    SeriesRun run{h, q, L_schedule, trace, temps, table.get(), sym, form == PER_WORLD_CONSTANTS, B, sizeof(StatsDev) * B, sizeof(TempStatsDev) * B};
    run.frames = frames;
    if (int rc = run.alloc()) return rc;
    SyncOnExit sync(h->stream);                                 // the downloads fill the caller's arrays
    h->fused_launches = 0;
    if (int rc = frames ? upload_selection(h, frames->sh) : DW_OK) return rc;
    if (int rc = run.run(rows.get())) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    sync.disarm();
    return DW_OK;
}

int dw_step_n_trace(dw_handle* h, int32_t nsteps, const double* L_schedule, dw_world_stats* trace) {
    NEED(h && L_schedule && trace, DW_EINVAL, "null argument");
    return run_series(h, nsteps, L_schedule, trace, nullptr, true, h->plan.trace_pairs);
}

int dw_step_n_trace_per_world(dw_handle* h, int32_t nsteps, const double* L_schedule, dw_world_stats* trace) {
    NEED(h && L_schedule, DW_EINVAL, "null argument");
    return run_series(h, nsteps, L_schedule, trace, nullptr, false, false, PER_WORLD_L);
}

int dw_world_params_of(const dw_handle* h, dw_world_params* out) {
    NEED(h && out, DW_EINVAL, "null argument");
    *out = world_params_of(h->prm);
    return DW_OK;
}

int dw_step_n_trace_ensemble(dw_handle* h, int32_t nsteps, const dw_world_params* worlds, const double* L_schedule,
                             dw_world_stats* trace, dw_temp_stats* temps) {
    static_assert(sizeof(dw_world_params) == 96, "dw_world_params layout");
    NEED(h && worlds && L_schedule, DW_EINVAL, "null argument");
    return run_series(h, nsteps, L_schedule, trace, temps, false, ensemble_pairs(h), PER_WORLD_CONSTANTS, worlds);
}

int dw_step_n_trace_temperature(dw_handle* h, int32_t nsteps, const double* L_schedule, int per_world, dw_world_stats* trace,
                                dw_temp_stats* temps) {
    NEED(h && L_schedule && temps, DW_EINVAL, "null argument");
    return run_series(h, nsteps, L_schedule, trace, temps, false, false, per_world ? PER_WORLD_L : SHARED_L);
}

int dw_reduce_tiles(dw_handle* h, double L, const dw_frame_spec* spec, dw_tile_cover* cover, double* temp_mean) {
    static_assert(sizeof(dw_tile_cover) == 8 && sizeof(dw_tile_cover) == sizeof(TileCoverDev), "tile record layout");
    NEED(h && spec, DW_EINVAL, "null argument");
    NEED(cover || temp_mean, DW_EINVAL, "neither cover nor temp_mean is wanted");
    FrameShape sh;
    if (int rc = check_frame_spec(h, spec, &sh)) return rc;
    if (int rc = check_luminosity(L, 0)) return rc;
    NEED(h->have_state, DW_ESTATE, "no state");
    NEED(!cover || cur_quantised(h), DW_ESTATE, "the current state is not quantised yet; take the first step with dw_step");
    if (temp_mean) NEED_SHARED_CONSTANTS(h, "dw_reduce_tiles");
    HIPCHK(hipSetDevice(h->prm.device));
    const size_t n = sh.records();
    if (int rc = alloc_group(h, "the frame buffers", {{h->frame_sel, sh.sel_bytes()}, {h->frame_cover, cover ? sizeof(TileCoverDev) * n : 0},
                                                       {h->frame_temp, temp_mean ? sizeof(double) * n : 0},
                                                       {h->tile_part, temp_mean ? sh.part_bytes() : 0}})) return rc;
    SyncOnExit sync(h->stream);                                 // the selection comes from the caller's array
    if (int rc = upload_selection(h, sh)) return rc;
    if (cover) {
        if (int rc = launch_tile_cover(h, sh, h->cur, h->frame_cover.get())) return rc;
        HIPCHK(hipMemcpyAsync(cover, h->frame_cover.get(), sizeof(TileCoverDev) * n, hipMemcpyDeviceToHost, h->stream));
    }
    if (temp_mean) {                                            // (the luminosity: run_materialise's rule - the caches' own)
        if (int rc = launch_tile_temp(h, false, h->stepped && !h->L_per_world ? h->L_last : L, sh, h->frame_temp.get())) return rc;
        HIPCHK(hipMemcpyAsync(temp_mean, h->frame_temp.get(), sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    sync.disarm();
    return DW_OK;
}

int dw_step_n_frames(dw_handle* h, int32_t nsteps, const double* L_schedule, const dw_frame_spec* spec, int32_t stride,
                     dw_tile_cover* cover, double* temp_mean, dw_world_stats* trace) {
    NEED(h && L_schedule && spec, DW_EINVAL, "null argument");
    NEED(cover || temp_mean, DW_EINVAL, "neither cover nor temp_mean is wanted");
    NEED(stride >= 1, DW_EINVAL, "stride < 1");
    NEED(nsteps >= 0, DW_EINVAL, "nsteps < 0");
    FrameRun frames{h, FrameShape{}, stride, cover, temp_mean};
    if (int rc = check_frame_spec(h, spec, &frames.sh)) return rc;
    for (int32_t t = 0; t < nsteps; ++t)
        if (int rc = check_luminosity(L_schedule[t], t)) return rc;
    return run_series(h, nsteps, L_schedule, trace, nullptr, true, h->plan.trace_pairs, SHARED_L, nullptr, &frames);
}

int dw_last_step_n_timing(dw_handle* h, float* fused_ms, int32_t* fused_launches, int32_t* plane_elem_bytes) {
    NEED(h && fused_ms && fused_launches && plane_elem_bytes, DW_EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->prm.device));
    *fused_ms = 0.f;
    *fused_launches = h->fused_launches;
    *plane_elem_bytes = (int32_t)sizeof(plane_t);
    if (h->fused_launches > 0) {
        HIPCHK(hipEventSynchronize(h->evf1));
        HIPCHK(hipEventElapsedTime(fused_ms, h->evf0, h->evf1));
    }
    return DW_OK;
}

int dw_forward_f64(dw_handle* h, const double* light, const double* dark, double L, double* grid7,
                   double* temps, double* betas, double* growth, double* temp_effective) {
    NEED(h && light && dark && grid7, DW_EINVAL, "null argument");
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    const size_t n = h->cells;
    // scratch layout: [in light n][in dark n][grid7 7n][caches 9n] doubles, [new light n][new dark n] binary16
    int rc = ensure_scratch(h, sizeof(double) * 18 * n + sizeof(plane_t) * 2 * n + 16);
    if (rc) return rc;
    double* dL = h->scratch.get();
    double* dD = dL + n;
    double* dG = dD + n;
    double* d_t = dG + 7 * n;
    double* d_b = d_t + 3 * n;
    double* d_g = d_b + 3 * n;
    double* d_e = d_g + 2 * n;
    plane_t* nL = reinterpret_cast<plane_t*>(d_e + n);
    plane_t* nD = nL + n;
    // the reductions of this side computation must not disturb the handle's per-world stats
    StatsDev* tmp_stats = h->side_stats.get();
    HIPCHK(hipMemsetAsync(tmp_stats, 0, sizeof(StatsDev) * (p.batch + 1), h->stream));
    HIPCHK(hipMemcpyAsync(dL, light, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
    {
        const hipError_t e2 = hipMemcpyAsync(dD, dark, sizeof(double) * n, hipMemcpyHostToDevice, h->stream);
        if (e2 != hipSuccess) {
            (void)hipStreamSynchronize(h->stream);      // the first copy may still be reading `light`
            return fail(DW_EHIP, "dw_forward_f64: %s", hipGetErrorString(e2));
        }
    }
    const PhysF32 P = derive_f32(p, L);
    const PhysF64 P64 = make_f64(p, L);
    unsigned long long* tmp_fix = &tmp_stats[p.batch].sum_l;
    for_world_slices(p.batch, [&](int b0, int nb) {
        const dim3 g((unsigned)((p.height * p.width + 255) / 256), (unsigned)nb);
        const size_t w = (size_t)b0 * p.height * p.width;
        hipLaunchKernelGGL((step_generic<double, 2>), g, dim3(256), 0, h->stream, dL + w, dD + w, nL + w, nD + w, p.height,
                           p.width, P, P64, tmp_stats + b0, tmp_fix, (unsigned long long*)nullptr, 0);
    });
    launch_materialise<double, true>(h, dL, dD, nL, nD, P64, dG, temps ? d_t : (double*)nullptr,
                                     betas ? d_b : (double*)nullptr, growth ? d_g : (double*)nullptr,
                                     temp_effective ? d_e : (double*)nullptr);
    hipError_t le = hipGetLastError();
    if (le == hipSuccess && p.n_agents && h->have_agents) {
        hipLaunchKernelGGL(agents_stamp, dim3((p.batch + 63) / 64), dim3(64), 0, h->stream, dG, h->idx.get(), h->st.get(),
                           p.batch, p.n_agents, p.height, p.width);
        le = hipGetLastError();
    }
    if (le == hipSuccess) le = hipMemcpyAsync(grid7, dG, sizeof(double) * 7 * n, hipMemcpyDeviceToHost, h->stream);
    if (le == hipSuccess && temps) le = hipMemcpyAsync(temps, d_t, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, h->stream);
    if (le == hipSuccess && betas) le = hipMemcpyAsync(betas, d_b, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, h->stream);
    if (le == hipSuccess && growth) le = hipMemcpyAsync(growth, d_g, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, h->stream);
    if (le == hipSuccess && temp_effective)
        le = hipMemcpyAsync(temp_effective, d_e, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream);
    // the caller's host buffers are the targets of copies in flight: never return before the stream is idle
    const hipError_t se = hipStreamSynchronize(h->stream);
    if (le == hipSuccess) le = se;
    if (le != hipSuccess) return fail(DW_EHIP, "dw_forward_f64: %s", hipGetErrorString(le));
    return DW_OK;
}

int dw_conv3x3_f64(dw_handle* h, const double* plane, const double kernel[9], double* out) {
    NEED(h && plane && kernel && out, DW_EINVAL, "null argument");
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    const size_t n = h->cells;
    int rc = ensure_scratch(h, sizeof(double) * 2 * n);
    if (rc) return rc;
    double* d_in = h->scratch.get();
    double* d_out = d_in + n;
    Kernel9 K;
    for (int i = 0; i < 9; ++i) K.k[i] = kernel[i];
    SyncOnExit guard(h->stream);                              // `plane` / `out` are the caller's
    HIPCHK(hipMemcpyAsync(d_in, plane, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
    for_world_slices(p.batch, [&](int b0, int nb) {
        const dim3 g((unsigned)((p.height * p.width + 255) / 256), (unsigned)nb);
        const size_t w = (size_t)b0 * p.height * p.width;
        hipLaunchKernelGGL(conv3x3_f64, g, dim3(256), 0, h->stream, d_in + w, d_out + w, p.height, p.width, K);
    });
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_out, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    guard.disarm();
    return DW_OK;
}

int dw_stage_f64(dw_handle* h, int stage, const double* in, double* out, double L, const double kernel[9]) {
    NEED(h && in && out, DW_EINVAL, "null argument");
    NEED(stage >= kStageAlbedo && stage <= kStageGrowth, DW_EINVAL, "bad stage %d", stage);
    NEED(kernel || stage > kStageDensity, DW_EINVAL, "the stencil stages need their 3x3 kernel");
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    const size_t n = h->cells, nin = (size_t)stage_inputs(stage), nout = (size_t)stage_outputs(stage);
    int rc = ensure_scratch(h, sizeof(double) * (nin + nout) * n);
    if (rc) return rc;
    double* d_in = h->scratch.get();
    double* d_out = d_in + nin * n;
    Kernel9 K{};
    if (kernel) for (int i = 0; i < 9; ++i) K.k[i] = kernel[i];
    const PhysF64 P = make_f64(p, L);
    SyncOnExit guard(h->stream);                              // `in` / `out` are the caller's
    HIPCHK(hipMemcpyAsync(d_in, in, sizeof(double) * nin * n, hipMemcpyHostToDevice, h->stream));
    with_int<kStageAlbedo, kStageDensity, kStageTemperature, kStageGrowthRate, kStageGrowth>(stage, [&](auto S) {
        for_world_slices(p.batch, [&](int b0, int nb) {          // (the kernel's B is the stride between planes: the batch's)
            const dim3 g((unsigned)((p.height * p.width + 255) / 256), (unsigned)nb);
            const size_t w = (size_t)b0 * p.height * p.width;
            hipLaunchKernelGGL((stage_f64<S>), g, dim3(256), 0, h->stream, d_in + w, d_out + w, p.batch, p.height, p.width, P, K);
        });
    });
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_out, sizeof(double) * nout * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    guard.disarm();
    return DW_OK;
}

int dw_get_obs(dw_handle* h, double L_init, double* obs) {
    NEED(h, DW_EINVAL, "null handle");
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    const size_t bn = (size_t)p.batch * p.n_agents;
    if (bn == 0) return DW_OK;
    NEED(obs, DW_EINVAL, "null obs");
    NEED(h->have_state && h->have_agents, DW_ESTATE, "no state / agents");
    int rc = observe_into_scratch(h, L_init, 0);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(obs, h->scratch.get(), sizeof(double) * bn * 63, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return DW_OK;
}

// step + get_obs + reward/done as one call.  Everything crosses PCIe through one page-locked staging
// buffer (pageable copies are staged and serialised by the runtime, ~20 us each): actions in, the three
// results out, all asynchronous on the handle's stream with ONE synchronisation.
int dw_env_step(dw_handle* h, const int32_t* action, int32_t action_b, int32_t action_n, double L, double* obs,
                double* reward, uint8_t* done) {
    NEED(h, DW_EINVAL, "null handle");
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    const size_t bn = (size_t)p.batch * p.n_agents;
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    const bool big_obs = sizeof(double) * bn * 63 > ((size_t)512 << 10);
    // pinned image: [actions | obs | reward | done] (the last three contiguous, as in the device block; for big
    // observation blocks only reward | done are staged, at o_rew)
    const size_t o_act = 0, o_obs = up(sizeof(int) * bn), o_rew = o_obs + sizeof(double) * bn * 63;
    const size_t total = up(o_rew + sizeof(double) * bn + bn) + 256;
    if (int rc = reserve(h->pinned, "the page-locked step staging", total)) return rc;
    if (action) {
        NEED(action_b >= 0 && action_n >= 0 && action_b <= p.batch && action_n <= p.n_agents, DW_EINVAL,
             "action block %dx%d exceeds (B,N)=(%d,%d)", action_b, action_n, p.batch, p.n_agents);
        const size_t na = (size_t)action_b * action_n;
        if (na) {
            std::memcpy(h->pinned.get() + o_act, action, sizeof(int) * na);
            HIPCHK(hipMemcpyAsync(h->action_tmp.get(), h->pinned.get() + o_act, sizeof(int) * na, hipMemcpyHostToDevice, h->stream));
        }
        int rc = launch_agents(h, h->action_tmp.get(), action_b, action_n);
        if (rc) return rc;
    }
    int rc = launch_forward(h, L);
    if (rc) return rc;
    if (bn) {
        NEED(h->have_agents, DW_ESTATE, "no agents");
        // observations, rewards and done flags land in ONE device block [obs | reward | done] and come back in
        // one copy (each extra copy costs its own ~5-10 us of latency on a 90 us step)
        const size_t d_rew = sizeof(double) * bn * 63, d_done = d_rew + sizeof(double) * bn, d_total = d_done + bn;
        rc = observe_into_scratch(h, L, d_total - d_rew + 64, true);     // reward | done written by the same kernel
        if (rc) return rc;
        unsigned char* blk = reinterpret_cast<unsigned char*>(h->scratch.get());
        if (big_obs) {
            if (obs) HIPCHK(hipMemcpyAsync(obs, blk, d_rew, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipMemcpyAsync(h->pinned.get() + o_rew, blk + d_rew, d_total - d_rew, hipMemcpyDeviceToHost, h->stream));
        } else {
            HIPCHK(hipMemcpyAsync(h->pinned.get() + o_obs, blk, d_total, hipMemcpyDeviceToHost, h->stream));
        }
        HIPCHK(hipStreamSynchronize(h->stream));
        const unsigned char* src = big_obs ? h->pinned.get() + o_rew - d_rew : h->pinned.get() + o_obs;     // base of the block image
        if (obs && !big_obs) std::memcpy(obs, src, d_rew);
        if (reward) std::memcpy(reward, src + d_rew, sizeof(double) * bn);
        if (done) std::memcpy(done, src + d_done, bn);
    }
    return DW_OK;
}

int dw_get_reward_done(dw_handle* h, double* reward, uint8_t* done) {
    NEED(h, DW_EINVAL, "null handle");
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    const int bn = p.batch * p.n_agents;
    if (bn == 0) return DW_OK;
    NEED(h->have_agents, DW_ESTATE, "no agents");
    hipLaunchKernelGGL(reward_done, dim3((bn + 255) / 256), dim3(256), 0, h->stream, h->st.get(), h->reward_d.get(), h->done_d.get(), bn);
    HIPCHK(hipGetLastError());
    if (reward) HIPCHK(hipMemcpyAsync(reward, h->reward_d.get(), sizeof(double) * bn, hipMemcpyDeviceToHost, h->stream));
    if (done) HIPCHK(hipMemcpyAsync(done, h->done_d.get(), (size_t)bn, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return DW_OK;
}

int dw_reduce(dw_handle* h, dw_world_stats* per_world) {
    NEED(h && per_world, DW_EINVAL, "null argument");
    NEED(h->have_state, DW_ESTATE, "no state");
    static_assert(sizeof(dw_world_stats) == sizeof(StatsDev), "stats layout");
    HIPCHK(hipSetDevice(h->prm.device));
    HIPCHK(hipMemcpyAsync(per_world, h->stats2[h->sp].get(), sizeof(StatsDev) * h->prm.batch, hipMemcpyDeviceToHost,
                          h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return DW_OK;
}

// Greedy / anti-greedy choice of every agent from the CURRENT covers (ref Greedy.__call__, agents/greedy.py:18-30)
// into h->action.get(); agent_mode / codes as in policy_greedy (dw_agents.hpp).
static int launch_policy_greedy(dw_handle* h, int argmin, const int* agent_mode, int codes) {
    const dw_params& p = h->prm;
    const int bn = p.batch * p.n_agents;
    const dim3 g((unsigned)((bn + 255) / 256));
    if (h->unq == OWN_CUR && h->unq_kind == UNQ_F32)
        hipLaunchKernelGGL(policy_greedy<float>, g, dim3(256), 0, h->stream, h->U32L.get(), h->U32D.get(), h->idx.get(), p.batch, p.n_agents,
                           p.height, p.width, p.obs_mask, argmin, agent_mode, h->action.get(), codes);
    else
        hipLaunchKernelGGL(policy_greedy<plane_t>, g, dim3(256), 0, h->stream, h->L16[h->cur].get(), h->D16[h->cur].get(), h->idx.get(),
                           p.batch, p.n_agents, p.height, p.width, p.obs_mask, argmin, agent_mode, h->action.get(), codes);
    HIPCHK(hipGetLastError());
    return DW_OK;
}

int dw_policy_greedy(dw_handle* h, int mode) {
    NEED(h, DW_EINVAL, "null handle");
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    const int bn = p.batch * p.n_agents;
    if (bn == 0) return DW_OK;
    NEED(h->have_state && h->have_agents, DW_ESTATE, "no state / agents");
    NEED(mode == DW_POLICY_ARGMAX || mode == DW_POLICY_ARGMIN, DW_EINVAL, "bad policy mode");
    NEED(cur_quantised(h) || h->unq_kind != UNQ_F64, DW_ESTATE,
         "device policy on an exact float64 initial state is not supported; compute the action on the host");
    return launch_policy_greedy(h, mode == DW_POLICY_ARGMIN ? 1 : 0, nullptr, 0);
}

int dw_policy_per_agent(dw_handle* h, const int32_t* agent_mode) {
    NEED(h && agent_mode, DW_EINVAL, "null argument");
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    const int bn = p.batch * p.n_agents;
    if (bn == 0) return DW_OK;
    NEED(h->have_state && h->have_agents, DW_ESTATE, "no state / agents");
    NEED(cur_quantised(h) || h->unq_kind != UNQ_F64, DW_ESTATE,
         "device policy on an exact float64 initial state is not supported; compute the action on the host");
    for (int n = 0; n < p.n_agents; ++n)
        NEED(agent_mode[n] == DW_POLICY_ARGMAX || agent_mode[n] == DW_POLICY_ARGMIN || agent_mode[n] == DW_POLICY_TABLE,
             DW_EINVAL, "agent %d: bad policy mode %d", n, agent_mode[n]);
    // modes travel in the (otherwise idle) staging buffer of host-supplied actions; 3 -> internal code 2
    std::vector<int> m(p.n_agents);
    for (int n = 0; n < p.n_agents; ++n) m[n] = agent_mode[n] == DW_POLICY_TABLE ? 2 : agent_mode[n];
    HIPCHK(hipMemcpyAsync(h->action_tmp.get(), m.data(), sizeof(int) * p.n_agents, hipMemcpyHostToDevice, h->stream));
    const int prc = launch_policy_greedy(h, 0, h->action_tmp.get(), 0);
    HIPCHK(hipStreamSynchronize(h->stream));      // `m` is a local host buffer: also on the error path
    return prc;
}

// fills h->scratch.get() with the [B][N][63] observations of the current state (device side of dw_get_obs)
// reward_tail: the kernel also writes [reward (B,N) float64 | done (B,N) u8] right behind the observations
static int observe_into_scratch(dw_handle* h, double L_init, size_t extra_bytes, bool reward_tail) {
    const dw_params& p = h->prm;
    const size_t bn = (size_t)p.batch * p.n_agents;
    NEED_SHARED_L(h, "an observation");
    int rc = ensure_scratch(h, sizeof(double) * bn * 63 + extra_bytes);
    if (rc) return rc;
    double* d_rew = reward_tail ? h->scratch.get() + bn * 63 : nullptr;
    unsigned char* d_done = reward_tail ? reinterpret_cast<unsigned char*>(h->scratch.get() + bn * 64) : nullptr;
    const int threads = (int)(bn * 9);
    const dim3 g((threads + 127) / 128);
    const PhysF64 P = make_f64(p, h->stepped ? h->L_last : L_init);
    const plane_t* cL = h->L16[h->cur].get();            // read by the POST variants only
    const plane_t* cD = h->D16[h->cur].get();
    with_derived_from(h, [&](auto* pL, auto* pD, auto POST) {
        hipLaunchKernelGGL((observe<elem_t<decltype(pL)>, POST>), g, dim3(128), 0, h->stream, pL, pD, cL, cD, h->idx.get(),
                           h->st.get(), p.batch, p.n_agents, p.height, p.width, P, p.obs_mask, h->scratch.get(), d_rew, d_done);
    });
    HIPCHK(hipGetLastError());
    return DW_OK;
}

static int policy_mlp_impl(dw_handle* h, const double* params, int32_t n_members, const int32_t* world_member,
                           int32_t agent_begin, int32_t agent_end, double L_init) {
    const dw_params& p = h->prm;
    NEED(agent_begin >= 0 && agent_begin <= agent_end && agent_end <= p.n_agents, DW_EINVAL, "bad agent range");
    NEED(h->have_state && h->have_agents, DW_ESTATE, "no state / agents");
    const size_t bn = (size_t)p.batch * p.n_agents;
    if (bn == 0 || agent_begin == agent_end) return DW_OK;
    if (world_member)
        for (int b = 0; b < p.batch; ++b)
            NEED(world_member[b] >= 0 && world_member[b] < n_members, DW_EINVAL, "world %d: member %d out of range", b,
                 world_member[b]);
    const size_t wbytes = sizeof(double) * 1808 * (size_t)n_members;
    const size_t mbytes = world_member ? sizeof(int) * (size_t)p.batch : 0;
    int rc = observe_into_scratch(h, L_init, wbytes + mbytes + 16);
    if (rc) return rc;
    double* d_w = h->scratch.get() + bn * 63;
    int* d_m = world_member ? reinterpret_cast<int*>(d_w + 1808 * (size_t)n_members) : nullptr;
    SyncOnExit guard(h->stream);                              // params / world_member are the caller's
    HIPCHK(hipMemcpyAsync(d_w, params, wbytes, hipMemcpyHostToDevice, h->stream));
    if (world_member) HIPCHK(hipMemcpyAsync(d_m, world_member, mbytes, hipMemcpyHostToDevice, h->stream));
    const int n = p.batch * (agent_end - agent_begin);
    hipLaunchKernelGGL(policy_mlp, dim3((n + 3) / 4), dim3(64), 0, h->stream, h->scratch.get(), d_w, d_m, p.batch,
                       p.n_agents, agent_begin, agent_end, h->action.get());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    guard.disarm();
    return DW_OK;
}

int dw_policy_mlp(dw_handle* h, const double* params, int32_t n_params, int32_t agent_begin, int32_t agent_end,
                  double L_init) {
    NEED(h && params, DW_EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->prm.device));
    NEED(n_params == 63 * 16 + 16 * 32 + 32 * 9, DW_EINVAL, "the MLP policy has 1808 parameters (63-16-32-9), got %d", n_params);
    return policy_mlp_impl(h, params, 1, nullptr, agent_begin, agent_end, L_init);
}

int dw_policy_mlp_population(dw_handle* h, const double* params, int32_t n_members, const int32_t* world_member,
                             int32_t agent_begin, int32_t agent_end, double L_init) {
    NEED(h && params && world_member, DW_EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->prm.device));
    NEED(n_members >= 1, DW_EINVAL, "n_members < 1");
    return policy_mlp_impl(h, params, n_members, world_member, agent_begin, agent_end, L_init);
}

// K steps with MLP policies without a host round trip: parameters and member maps go to the device once;
// per step: observe (all agents) -> policy_mlp for [0, split) and [split, N) -> update_agents -> step ->
// reward / done of the step into the [K][B][N] device buffers; one download and synchronisation at the end.
// `trace` / `temps` (dw_run_episode_mlp_trace; either may be null): also the records of every step and the temperature
// records, [K][B] each, in the TRACE region of the staging buffer.  The one-wave-per-world form takes
// episode_mlp_wave_trace_pw<EXACT, temps given>; every other form - and the first steps of an episode - launches per step,
// with temp_moments_pw on the grazed current state (in its own format while it is the un-quantised upload) in front of the
// step kernel and episode_stats_row_pw behind it: no LDS workgroup kernel, the stated price of the records.
// `account_fitness` (dw_run_episode_mlp_fitness): the fitness bookkeeping of the chunk goes on the stream behind its last
// step, in front of the downloads and the one synchronisation - it reads the rewards and flags where the steps left them;
// its scratch is allocated behind this call's checks, with the staging buffer.
static int ensure_fitness_scratch(dw_handle* h, size_t K);
static int launch_fitness_account(dw_handle* h, size_t K, const double* d_reward, const unsigned char* d_done);
static int run_episode_mlp_impl(dw_handle* h, int32_t nsteps, const double* L_schedule, const double* params, int32_t n_members,
                                const int32_t* member_a, const int32_t* member_b, int32_t split, double L_init, double* reward,
                                uint8_t* done, dw_world_stats* trace, dw_temp_stats* temps, bool account_fitness = false) {
    const bool records = trace || temps;
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    NEED(nsteps >= 1 && nsteps <= 4096, DW_EINVAL, "nsteps must be in 1..4096");
    NEED(n_members >= 1, DW_EINVAL, "n_members < 1");
    NEED(params || (h->mlp_w.get() && h->mlp_members == n_members), DW_ESTATE,
         "params == NULL but no parameter sets of %d members are on the device", n_members);
    NEED(p.collision_mode == 0, DW_EINVAL, "collision_mode=1 is not implemented on the device");
    NEED(split >= 0 && split <= p.n_agents, DW_EINVAL, "split outside 0..n_agents");
    NEED(h->have_state && h->have_agents, DW_ESTATE, "no state / agents");
    const int B = p.batch, N = p.n_agents;
    const size_t K = (size_t)nsteps, bn = (size_t)B * N;
    NEED(bn > 0, DW_EINVAL, "no agents");
    for (int b = 0; b < B; ++b) {
        NEED(!member_a || (member_a[b] >= 0 && member_a[b] < n_members), DW_EINVAL, "world %d: member out of range", b);
        NEED(!member_b || (member_b[b] >= 0 && member_b[b] < n_members), DW_EINVAL, "world %d: member out of range", b);
    }
    NEED(n_members == 1 || (member_a && member_b), DW_EINVAL, "several parameter sets need both member maps");
    // every step observes first: refused here, before the caller's sets replace the resident ones (a refused call leaves
    // the handle as it was, the parameter sets a later params == NULL relies on included)
    NEED_SHARED_L(h, "the episode's first observation");
    const size_t wbytes = sizeof(double) * 1808 * (size_t)n_members;
    EpisodeRegions regions;
    regions.rows = K; regions.mlp = true; regions.trace = records; regions.temps = temps != nullptr;
    const EpisodeStaging S(K, (size_t)B, (size_t)N, regions);
    using R = EpisodeStaging;
    const size_t o_ma = S.off[R::MEMBER_A], o_mb = S.off[R::MEMBER_B], o_p32 = S.off[R::P32], o_ls = S.off[R::LS];
    if (temps)                                                  // the partials of temp_moments_pw (the rows live in the staging buffer)
        if (int rc = alloc_group(h, "the temperature reduction", {{h->temp_part, temp_part_bytes(h)}})) return rc;
    if (account_fitness)
        if (int rc = ensure_fitness_scratch(h, K)) return rc;
    if (int erc = ensure_ep_buf(h, S.total)) return erc;
    if (params) {                                               // the sets stay on the device for later calls (params == NULL)
        if (h->mlp_members != n_members) {
            h->mlp_w.reset();
            h->mlp_members = 0;
            if (int rc = reserve(h->mlp_w, "the parameter sets", wbytes)) return rc;
            h->mlp_members = n_members;
        }
    }
    const double* d_w = h->mlp_w.get();
    const int* d_ma = member_a ? reinterpret_cast<const int*>(h->ep_buf.get() + o_ma) : nullptr;
    const int* d_mb = member_b ? reinterpret_cast<const int*>(h->ep_buf.get() + o_mb) : nullptr;
    double* d_r = S.at<double>(h->ep_buf.get(), R::REWARD);
    unsigned char* d_d = S.at<unsigned char>(h->ep_buf.get(), R::DONE);
    StatsDev* const d_rows = S.at<StatsDev>(h->ep_buf.get(), R::TRACE);
    TempStatsDev* const d_trows = reinterpret_cast<TempStatsDev*>(h->ep_buf.get() + S.temps_off());
    SyncOnExit guard(h->stream);                              // params / member maps are the caller's
    if (params) HIPCHK(hipMemcpyAsync(h->mlp_w.get(), params, wbytes, hipMemcpyHostToDevice, h->stream));
    if (member_a) HIPCHK(hipMemcpyAsync(h->ep_buf.get() + o_ma, member_a, sizeof(int) * B, hipMemcpyHostToDevice, h->stream));
    if (member_b) HIPCHK(hipMemcpyAsync(h->ep_buf.get() + o_mb, member_b, sizeof(int) * B, hipMemcpyHostToDevice, h->stream));
    // Small worlds with a quantised state and a quantised retained previous state: the rest of the chunk in ONE
    // launch, worlds in LDS (episode_mlp).  Until then - the first two steps of an episode, whose current /
    // previous state is the un-quantised upload - and for large worlds: one launch sequence per step.
    const int Cc = p.height * p.width;
    const int wpb = worlds_per_block(Cc);
    size_t lds = 0;
    const EpisodeForm form = episode_mlp_form(h, &lds);
    const bool wave_kernel = form == EPISODE_WAVE, small = records ? form == EPISODE_WAVE : form != EPISODE_STEPWISE;
    if (records) lds = episode_mlp_wave_trace_lds_bytes(Cc, N);
    std::vector<PhysF32> p32;
    SyncOnExit guard2(h->stream);                             // p32 (filled below) must outlive its upload
    size_t t = 0;
    while (t < K) {
        if (small && cur_quantised(h) && h->stepped && h->unq == OWN_NONE) {
            NEED_SHARED_L(h, "the episode's first observation");
            const size_t Kr = K - t;
            p32.resize(Kr);
            for (size_t i = 0; i < Kr; ++i) p32[i] = derive_f32(p, L_schedule[t + i]);
            HIPCHK(hipMemcpyAsync(h->ep_buf.get() + o_p32, p32.data(), sizeof(PhysF32) * Kr, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(h->ep_buf.get() + o_ls, L_schedule + t, sizeof(double) * Kr, hipMemcpyHostToDevice, h->stream));
            StatsDev* stats = h->stats2[h->sp].get();
            if (!wave_kernel) HIPCHK(hipMemsetAsync(stats, 0, sizeof(StatsDev) * (B + 1), h->stream));   // (the wave kernel assigns every record)
            EpisodeMlpIO io;
            fill_episode_io(io, h, S);
            io.weights = d_w; io.member_a = d_ma; io.member_b = d_mb;
            io.reward = d_r + t * bn; io.done = d_d + t * bn;
            io.action = h->action.get();
            const bool ex = p.precision == DW_PRECISION_EXACT;
            if (records) {
                auto kern = temps ? (ex ? episode_mlp_wave_trace_pw<true, true> : episode_mlp_wave_trace_pw<false, true>)
                                  : (ex ? episode_mlp_wave_trace_pw<true, false> : episode_mlp_wave_trace_pw<false, false>);
                if (int rc = set_lds_limit(h, kern, lds)) return rc;
                const EpisodeMlpWaveTraceArgs A{io, d_rows + t * B, temps ? d_trows + t * B : nullptr, B, N, p.height, p.width,
                                                (int)Kr, p.obs_mask, (int)split, p.agent_gamma, h->L_last,
                                                make_f64(p, L_schedule[t])};
                hipLaunchKernelGGL(kern, dim3((unsigned)((B + 3) / 4)), dim3(256), lds, h->stream, A);
            } else if (wave_kernel) {
                auto kern = ex ? episode_mlp_wave<true> : episode_mlp_wave<false>;
                if (int rc = set_lds_limit(h, kern, lds)) return rc;
                const EpisodeMlpWaveArgs A{io, B, N, p.height, p.width, (int)Kr, p.obs_mask, (int)split, p.agent_gamma,
                                           h->L_last, make_f64(p, L_schedule[t])};
                hipLaunchKernelGGL(kern, dim3((unsigned)((B + 3) / 4)), dim3(256), lds, h->stream, A);
            } else {
                auto kern = ex ? episode_mlp<true> : episode_mlp<false>;
                if (int rc = set_lds_limit(h, kern, lds)) return rc;
                hipLaunchKernelGGL(kern, dim3((unsigned)((B + wpb - 1) / wpb)), dim3(256), lds, h->stream, io, B, N, p.height,
                                   p.width, wpb, (int)Kr, p.obs_mask, p.agent_gamma, make_f64(p, L_schedule[t]), h->L_last,
                                   (int)split);
            }
            HIPCHK(hipGetLastError());
            h->stepped = true;
            h->L_last = L_schedule[K - 1];
            h->L_per_world = false;
            t = K;
            break;
        }
        int rc = observe_into_scratch(h, L_init, 0);
        if (rc) return rc;
        // both halves in one launch (agents [split, N) read member_b), reward / done written by the grazing
        // kernel: 4 instead of 6 launches per step - the loop is bound by the host thread that issues them
        hipLaunchKernelGGL(policy_mlp, dim3((unsigned)((bn + 3) / 4)), dim3(64), 0, h->stream, h->scratch.get(), d_w, d_ma, B, N,
                           0, N, h->action.get(), d_mb, split);
        HIPCHK(hipGetLastError());
        rc = launch_agents(h, h->action.get(), B, N, false, d_r + t * bn, d_d + t * bn);
        if (rc) return rc;
        if (temps) {                                            // the field this step computes: after its grazing, at its luminosity
            rc = launch_temp_moments(h, /*current=*/true, L_schedule[t], nullptr, d_trows + t * B);
            if (rc) return rc;
        }
        rc = launch_forward(h, L_schedule[t]);
        if (rc) return rc;
        if (trace) {
            hipLaunchKernelGGL(episode_stats_row_pw, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream,
                               h->stats2[h->sp].get(), B, d_rows + t * B);
            HIPCHK(hipGetLastError());
        }
        ++t;
    }
    if (account_fitness)
        if (int rc = launch_fitness_account(h, K, d_r, d_d)) return rc;
    if (reward) HIPCHK(hipMemcpyAsync(reward, d_r, sizeof(double) * K * bn, hipMemcpyDeviceToHost, h->stream));
    if (done) HIPCHK(hipMemcpyAsync(done, d_d, K * bn, hipMemcpyDeviceToHost, h->stream));
    if (trace) HIPCHK(hipMemcpyAsync(trace, d_rows, S.stats_bytes, hipMemcpyDeviceToHost, h->stream));
    if (temps) HIPCHK(hipMemcpyAsync(temps, d_trows, S.temps_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    guard2.disarm();
    guard.disarm();
    return DW_OK;
}

int dw_run_episode_mlp(dw_handle* h, int32_t nsteps, const double* L_schedule, const double* params, int32_t n_members,
                       const int32_t* member_a, const int32_t* member_b, int32_t split, double L_init, double* reward,
                       uint8_t* done) {
    NEED(h && L_schedule, DW_EINVAL, "null argument");
    return run_episode_mlp_impl(h, nsteps, L_schedule, params, n_members, member_a, member_b, split, L_init, reward, done, nullptr,
                                nullptr);
}

// ---- dw_run_episode_mlp_trace: dw_run_episode_mlp with the records of every step -----------------------------------------
// The form the call takes: one wave per world (episode_mlp_wave_trace_pw) wherever dw_run_episode_mlp takes episode_mlp_wave;
// every other shape, DW_NO_EPISODE_WAVE and DW_NO_EPISODE_KERNEL: launches per step.  Both reduce the temperature field in
// temp_moments_pw's order: the same bytes.
int dw_run_episode_mlp_trace(dw_handle* h, int32_t nsteps, const double* L_schedule, const double* params, int32_t n_members,
                             const int32_t* member_a, const int32_t* member_b, int32_t split, double L_init, double* reward,
                             uint8_t* done, dw_world_stats* trace, dw_temp_stats* temps) {
    NEED(h && L_schedule, DW_EINVAL, "null argument");
    NEED(trace || temps, DW_EINVAL, "dw_run_episode_mlp_trace needs a trace or a temps array (rewards only: dw_run_episode_mlp)");
    static_assert(sizeof(dw_temp_stats) == sizeof(TempStatsDev) && sizeof(TempStatsDev) == EpisodeStaging::kTempRow, "temperature record layout");
    static_assert(sizeof(dw_world_stats) == sizeof(StatsDev), "record layout");
    return run_episode_mlp_impl(h, nsteps, L_schedule, params, n_members, member_a, member_b, split, L_init, reward, done, trace,
                                temps);
}

// ---- dw_run_episode_mlp_counts: dw_run_episode_mlp_trace (cover records) with a number of agents per world ----------------
// run_episode_mlp_impl's chain with the counts: the states of absent agents are zeroed once; then, once the current and the
// retained previous state are quantised, the rest of the chunk in ONE launch of episode_mlp_counts_pw (where
// dw_counts_plan.hpp says so); until then and everywhere else per step observe_counts_pw -> policy_mlp (zero rows: action
// 0) -> grazing (a state-0 agent is inert) -> the step kernel -> episode_stats_row_pw.  Both forms leave the same bytes.
int dw_run_episode_mlp_counts(dw_handle* h, int32_t nsteps, const double* L_schedule, const double* params, int32_t n_members,
                              const int32_t* member_a, const int32_t* member_b, int32_t split, const int32_t* n_active,
                              double L_init, double* reward, uint8_t* done, dw_world_stats* trace) {
    NEED(n_active, DW_EINVAL, "n_active is null");
    NEED(h && L_schedule, DW_EINVAL, "null argument");
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    NEED(nsteps >= 1 && nsteps <= 4096, DW_EINVAL, "nsteps must be in 1..4096");
    NEED(n_members >= 1, DW_EINVAL, "n_members < 1");
    NEED(params || (h->mlp_w.get() && h->mlp_members == n_members), DW_ESTATE,
         "params == NULL but no parameter sets of %d members are on the device", n_members);
    NEED(p.collision_mode == 0, DW_EINVAL, "collision_mode=1 is not implemented on the device");
    NEED(p.precision != DW_PRECISION_F64, DW_EINVAL, "dw_run_episode_mlp_counts takes DW_PRECISION_EXACT and DW_PRECISION_FAST");
    NEED(split >= 0 && split <= p.n_agents, DW_EINVAL, "split outside 0..n_agents");
    NEED(h->have_state && h->have_agents, DW_ESTATE, "no state / agents");
    const int B = p.batch, N = p.n_agents;
    const size_t K = (size_t)nsteps, bn = (size_t)B * N;
    NEED(bn > 0, DW_EINVAL, "no agents");
    for (int b = 0; b < B; ++b) {
        NEED(!member_a || (member_a[b] >= 0 && member_a[b] < n_members), DW_EINVAL, "world %d: member out of range", b);
        NEED(!member_b || (member_b[b] >= 0 && member_b[b] < n_members), DW_EINVAL, "world %d: member out of range", b);
        NEED(n_active[b] >= 0 && n_active[b] <= N, DW_EINVAL, "world %d: %d agents, outside 0..%d", b, n_active[b], N);
    }
    NEED(n_members == 1 || (member_a && member_b), DW_EINVAL, "several parameter sets need both member maps");
    NEED_SHARED_L(h, "the episode's first observation");
    const size_t wbytes = sizeof(double) * 1808 * (size_t)n_members;
    EpisodeRegions regions;
    regions.rows = K; regions.mlp = true; regions.trace = trace != nullptr;
    const EpisodeStaging S(K, (size_t)B, (size_t)N, regions);
    using R = EpisodeStaging;
    const size_t o_ma = S.off[R::MEMBER_A], o_mb = S.off[R::MEMBER_B], o_p32 = S.off[R::P32], o_ls = S.off[R::LS];
    if (int rc = alloc_group(h, "the agent counts", {{h->n_active_d, sizeof(int) * (size_t)B}})) return rc;
    if (int rc = ensure_scratch(h, sizeof(double) * bn * 63)) return rc;
    if (int rc = ensure_ep_buf(h, S.total)) return rc;
    if (params && h->mlp_members != n_members) {                // the sets stay on the device for later calls (params == NULL)
        h->mlp_w.reset();
        h->mlp_members = 0;
        if (int rc = reserve(h->mlp_w, "the parameter sets", wbytes)) return rc;
        h->mlp_members = n_members;
    }
    const double* d_w = h->mlp_w.get();
    const int* d_na = h->n_active_d.get();
    const int* d_ma = member_a ? reinterpret_cast<const int*>(h->ep_buf.get() + o_ma) : nullptr;
    const int* d_mb = member_b ? reinterpret_cast<const int*>(h->ep_buf.get() + o_mb) : nullptr;
    double* d_r = S.at<double>(h->ep_buf.get(), R::REWARD);
    unsigned char* d_d = S.at<unsigned char>(h->ep_buf.get(), R::DONE);
    StatsDev* const d_rows = S.at<StatsDev>(h->ep_buf.get(), R::TRACE);
    SyncOnExit guard(h->stream);                              // params / member maps / counts are the caller's
    if (params) HIPCHK(hipMemcpyAsync(h->mlp_w.get(), params, wbytes, hipMemcpyHostToDevice, h->stream));
    if (member_a) HIPCHK(hipMemcpyAsync(h->ep_buf.get() + o_ma, member_a, sizeof(int) * B, hipMemcpyHostToDevice, h->stream));
    if (member_b) HIPCHK(hipMemcpyAsync(h->ep_buf.get() + o_mb, member_b, sizeof(int) * B, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->n_active_d.get(), n_active, sizeof(int) * B, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(zero_absent_states_pw, dim3((unsigned)((bn + 255) / 256)), dim3(256), 0, h->stream, h->st.get(), d_na, B, N);
    HIPCHK(hipGetLastError());
    const int Cc = p.height * p.width;
    const int wpb = counts_worlds_per_block(Cc);
    const bool small = episode_mlp_counts_workgroup(h);
    const size_t lds = episode_mlp_counts_dynamic_lds(Cc, N);
    std::vector<PhysF32> p32;
    SyncOnExit guard2(h->stream);                             // p32 (filled below) must outlive its upload
    size_t t = 0;
    while (t < K) {
        if (small && cur_quantised(h) && h->stepped && h->unq == OWN_NONE) {
            const size_t Kr = K - t;
            p32.resize(Kr);
            for (size_t i = 0; i < Kr; ++i) p32[i] = derive_f32(p, L_schedule[t + i]);
            HIPCHK(hipMemcpyAsync(h->ep_buf.get() + o_p32, p32.data(), sizeof(PhysF32) * Kr, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(h->ep_buf.get() + o_ls, L_schedule + t, sizeof(double) * Kr, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemsetAsync(h->stats2[h->sp].get(), 0, sizeof(StatsDev) * (B + 1), h->stream));
            EpisodeMlpCountsArgs A;
            fill_episode_io(A.io, h, S);
            A.io.weights = d_w; A.io.member_a = d_ma; A.io.member_b = d_mb;
            A.io.reward = d_r + t * bn; A.io.done = d_d + t * bn;
            A.io.action = h->action.get();
            A.n_active = d_na;
            A.trace = trace ? d_rows + t * B : nullptr;
            A.B = B; A.N = N; A.H = p.height; A.W = p.width; A.wpb = wpb; A.K = (int)Kr; A.obs_mask = p.obs_mask; A.split = (int)split;
            A.agent_gamma = p.agent_gamma; A.L_prev0 = h->L_last; A.P64 = make_f64(p, L_schedule[t]);
            auto kern = p.precision == DW_PRECISION_EXACT ? episode_mlp_counts_pw<true> : episode_mlp_counts_pw<false>;
            if (int rc = set_lds_limit(h, kern, lds)) return rc;
            hipLaunchKernelGGL(kern, dim3((unsigned)((B + wpb - 1) / wpb)), dim3(kCountsThreads), lds, h->stream, A);
            HIPCHK(hipGetLastError());
            h->stepped = true;
            h->L_last = L_schedule[K - 1];
            h->L_per_world = false;
            t = K;
            break;
        }
        {                                                       // observe_into_scratch with the counts
            NEED_SHARED_L(h, "an observation");
            const dim3 g((unsigned)((bn * 9 + 127) / 128));
            const PhysF64 P = make_f64(p, h->stepped ? h->L_last : L_init);
            const plane_t* cL = h->L16[h->cur].get();          // read by the POST variants only
            const plane_t* cD = h->D16[h->cur].get();
            with_derived_from(h, [&](auto* pL, auto* pD, auto POST) {
                hipLaunchKernelGGL((observe_counts_pw<elem_t<decltype(pL)>, POST>), g, dim3(128), 0, h->stream, pL, pD, cL, cD,
                                   h->idx.get(), h->st.get(), d_na, B, N, p.height, p.width, P, p.obs_mask, h->scratch.get());
            });
            HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(policy_mlp, dim3((unsigned)((bn + 3) / 4)), dim3(64), 0, h->stream, h->scratch.get(), d_w, d_ma, B, N,
                           0, N, h->action.get(), d_mb, split);
        HIPCHK(hipGetLastError());
        int rc = launch_agents(h, h->action.get(), B, N, false, d_r + t * bn, d_d + t * bn);
        if (rc) return rc;
        rc = launch_forward(h, L_schedule[t]);
        if (rc) return rc;
        if (trace) {
            hipLaunchKernelGGL(episode_stats_row_pw, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream,
                               h->stats2[h->sp].get(), B, d_rows + t * B);
            HIPCHK(hipGetLastError());
        }
        ++t;
    }
    if (reward) HIPCHK(hipMemcpyAsync(reward, d_r, sizeof(double) * K * bn, hipMemcpyDeviceToHost, h->stream));
    if (done) HIPCHK(hipMemcpyAsync(done, d_d, K * bn, hipMemcpyDeviceToHost, h->stream));
    if (trace) HIPCHK(hipMemcpyAsync(trace, d_rows, S.stats_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    guard2.disarm();
    guard.disarm();
    return DW_OK;
}

// ---- dw_fitness_*: the bookkeeping of a population's fitness episodes on the device (dw_fitness.hpp) -------------------------
// P = B / worlds_per_member members; the accumulators stay on the device from dw_fitness_begin to dw_fitness_download, a
// chunk brings (executed, finished) down and nothing else.
static int fitness_members(const dw_handle* h) { return h->prm.batch / h->fit_wpm; }

static int check_fitness_chunk(const dw_handle* h, int32_t nsteps) {
    NEED(nsteps >= 1 && nsteps <= 4096, DW_EINVAL, "nsteps must be in 1..4096");
    NEED(h->fit_wpm > 0, DW_ESTATE, "no dw_fitness_begin on this handle yet");
    return DW_OK;
}

// the scratch of a chunk of K steps: one group, all or nothing
static int ensure_fitness_scratch(dw_handle* h, size_t K) {
    const size_t kp = K * (size_t)fitness_members(h);
    return alloc_group(h, "the fitness bookkeeping of a chunk",
                       {{h->fit_means, sizeof(double) * kp}, {h->fit_all_done, kp}, {h->fit_run_t, kp}});
}

// The three launches of a chunk whose rewards and flags are on the device, and the copy of (executed, finished) into the
// page-locked words: the caller synchronises and reads them with fitness_outcome.
static int launch_fitness_account(dw_handle* h, size_t K, const double* d_reward, const unsigned char* d_done) {
    const dw_params& p = h->prm;
    const int P = fitness_members(h);
    const FitnessArgs A{d_reward, d_done, (int)K, p.batch, p.n_agents, h->fit_wpm, h->fit_half, P,
                        h->fit_means.get(), h->fit_all_done.get(), h->fit_run_t.get(), h->fit_out.get(),
                        h->fit_sum.get(), h->fit_done_at.get(), h->fit_running.get()};
    const size_t kp = K * (size_t)P, bn = (size_t)p.batch * p.n_agents;
    hipLaunchKernelGGL(fitness_means_pw, dim3((unsigned)((kp + kFitGroups - 1) / kFitGroups)), dim3(256), 0, h->stream, A);
    hipLaunchKernelGGL(fitness_scan_pw, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, h->stream, A);
    hipLaunchKernelGGL(fitness_counts_pw, dim3((unsigned)((bn + 255) / 256)), dim3(256), 0, h->stream, A);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h->fit_out_host.get(), h->fit_out.get() + 1, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    return DW_OK;
}

static void fitness_outcome(const dw_handle* h, int32_t* executed, int32_t* finished) {
    if (executed) *executed = h->fit_out_host.get()[0];
    if (finished) *finished = h->fit_out_host.get()[1];
}

int dw_fitness_begin(dw_handle* h, int32_t worlds_per_member, int32_t half) {
    NEED(h, DW_EINVAL, "null handle");
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    NEED(worlds_per_member >= 1 && p.batch % worlds_per_member == 0, DW_EINVAL,
         "worlds_per_member (%d) must divide the batch (%d)", worlds_per_member, p.batch);
    NEED(half >= 1 && half <= p.n_agents, DW_EINVAL, "half (%d) outside 1..n_agents (%d)", half, p.n_agents);
    const size_t P = (size_t)(p.batch / worlds_per_member), bn = (size_t)p.batch * p.n_agents;
    NEED(bn <= (size_t)0x7fffffff, DW_EINVAL, "the fitness bookkeeping indexes B * N with 32 bits");
    if (int rc = alloc_group(h, "the fitness accumulators", {{h->fit_sum, sizeof(double) * P}, {h->fit_done_at, sizeof(int) * bn},
                                                              {h->fit_running, P}, {h->fit_out, 3 * sizeof(int)}})) {
        h->fit_wpm = 0;                                         // nothing of an earlier begin is left to account into
        return rc;
    }
    if (int rc = reserve(h->fit_out_host, "the page-locked fitness outcome", 2 * sizeof(int))) return rc;
    HIPCHK(hipMemsetAsync(h->fit_sum.get(), 0, sizeof(double) * P, h->stream));
    HIPCHK(hipMemsetAsync(h->fit_done_at.get(), 0, sizeof(int) * bn, h->stream));
    HIPCHK(hipMemsetAsync(h->fit_running.get(), 1, P, h->stream));
    HIPCHK(hipMemsetAsync(h->fit_out.get(), 0, 3 * sizeof(int), h->stream));
    h->fit_wpm = worlds_per_member;
    h->fit_half = half;
    return DW_OK;
}

int dw_fitness_account(dw_handle* h, int32_t nsteps, const double* reward, const uint8_t* done, int32_t* executed,
                       int32_t* finished) {
    NEED(h && reward && done, DW_EINVAL, "null argument");
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    if (int rc = check_fitness_chunk(h, nsteps)) return rc;
    const size_t K = (size_t)nsteps, bn = (size_t)p.batch * p.n_agents;
    EpisodeRegions regions;
    regions.mlp = true;                                         // the REWARD and DONE regions of a dw_run_episode_mlp chunk
    const EpisodeStaging S(K, (size_t)p.batch, (size_t)p.n_agents, regions);
    if (int rc = ensure_fitness_scratch(h, K)) return rc;
    if (int rc = ensure_ep_buf(h, S.total)) return rc;
    double* d_r = S.at<double>(h->ep_buf.get(), EpisodeStaging::REWARD);
    unsigned char* d_d = S.at<unsigned char>(h->ep_buf.get(), EpisodeStaging::DONE);
    SyncOnExit guard(h->stream);                              // reward / done are the caller's
    HIPCHK(hipMemcpyAsync(d_r, reward, sizeof(double) * K * bn, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_d, done, K * bn, hipMemcpyHostToDevice, h->stream));
    if (int rc = launch_fitness_account(h, K, d_r, d_d)) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    guard.disarm();
    fitness_outcome(h, executed, finished);
    return DW_OK;
}

int dw_run_episode_mlp_fitness(dw_handle* h, int32_t nsteps, const double* L_schedule, const double* params, int32_t n_members,
                               const int32_t* member_a, const int32_t* member_b, int32_t split, double L_init,
                               int32_t* executed, int32_t* finished) {
    NEED(h && L_schedule, DW_EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->prm.device));
    if (int rc = check_fitness_chunk(h, nsteps)) return rc;
    if (int rc = run_episode_mlp_impl(h, nsteps, L_schedule, params, n_members, member_a, member_b, split, L_init, nullptr, nullptr,
                                      nullptr, nullptr, /*account_fitness=*/true))
        return rc;
    fitness_outcome(h, executed, finished);
    return DW_OK;
}

int dw_fitness_download(dw_handle* h, double* sum_reward, int32_t* done_at, uint8_t* running) {
    NEED(h, DW_EINVAL, "null handle");
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    NEED(h->fit_wpm > 0, DW_ESTATE, "no dw_fitness_begin on this handle yet");
    const size_t P = (size_t)fitness_members(h), bn = (size_t)p.batch * p.n_agents;
    if (sum_reward) HIPCHK(hipMemcpyAsync(sum_reward, h->fit_sum.get(), sizeof(double) * P, hipMemcpyDeviceToHost, h->stream));
    if (done_at) HIPCHK(hipMemcpyAsync(done_at, h->fit_done_at.get(), sizeof(int) * bn, hipMemcpyDeviceToHost, h->stream));
    if (running) HIPCHK(hipMemcpyAsync(running, h->fit_running.get(), P, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return DW_OK;
}

int dw_lifespan_reset(dw_handle* h) {
    NEED(h, DW_EINVAL, "null handle");
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    const size_t bn = (size_t)p.batch * (p.n_agents > 0 ? p.n_agents : 1);
    HIPCHK(hipMemsetAsync(h->done_at.get(), 0, sizeof(int) * p.batch, h->stream));
    HIPCHK(hipMemsetAsync(h->agents_done_at.get(), 0, sizeof(int) * bn, h->stream));
    HIPCHK(hipMemsetAsync(h->n_alive.get(), 0, sizeof(int), h->stream));
    return DW_OK;
}

int dw_lifespan_accumulate(dw_handle* h, uint32_t threshold_k) {
    NEED(h, DW_EINVAL, "null handle");
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    HIPCHK(hipMemsetAsync(h->n_alive.get(), 0, sizeof(int), h->stream));
    const int n = p.batch * (p.n_agents > 0 ? p.n_agents : 1);
    hipLaunchKernelGGL(lifespan_accumulate, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->stats2[h->sp].get(), h->st.get(), p.batch,
                       p.n_agents, threshold_k, h->done_at.get(), h->agents_done_at.get(), h->n_alive.get());
    HIPCHK(hipGetLastError());
    return DW_OK;
}

int dw_lifespan_download(dw_handle* h, int32_t* done_at, int32_t* agents_done_at, int32_t* n_worlds_alive) {
    NEED(h, DW_EINVAL, "null handle");
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    if (done_at) HIPCHK(hipMemcpyAsync(done_at, h->done_at.get(), sizeof(int) * p.batch, hipMemcpyDeviceToHost, h->stream));
    if (agents_done_at && p.n_agents)
        HIPCHK(hipMemcpyAsync(agents_done_at, h->agents_done_at.get(), sizeof(int) * (size_t)p.batch * p.n_agents,
                              hipMemcpyDeviceToHost, h->stream));
    if (n_worlds_alive) HIPCHK(hipMemcpyAsync(n_worlds_alive, h->n_alive.get(), sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return DW_OK;
}

int dw_run_episode(dw_handle* h, int32_t nsteps, const double* L_schedule, int policy_mode,
                   const uint8_t* use_table, const int8_t* table, uint32_t threshold_k, uint8_t* world_alive,
                   uint8_t* agent_ok) {
    NEED(h && L_schedule, DW_EINVAL, "null argument");
    NEED(policy_mode >= 0 && policy_mode <= 3, DW_EINVAL, "bad policy mode");
    return run_episode_impl(h, nsteps, L_schedule, policy_mode, use_table, table, threshold_k, world_alive, agent_ok);
}

// dw_run_episode (and the agent-free runs dw_step_n hands to it).  DW_PRECISION_F64 and collision_mode 1 have no
// LDS-resident kernel: dw_step_n launches per step, dw_run_episode itself rejects them.
static EpisodeForm episode_form(const dw_handle* h) {
    const dw_params& p = h->prm;
    const int C = p.height * p.width, N = p.n_agents;
    if (C > 4096 || p.precision == DW_PRECISION_F64 || p.collision_mode != 0 || h->sw.no_episode_kernel)
        return EPISODE_STEPWISE;
    // H*W <= 256 (the README sweep's 8x8, the ES trainers' 16x16): one wave per world (dw_episode_wave.hpp)
    return C <= kEwMaxCells && N <= 64 && !h->sw.no_episode_wave ? EPISODE_WAVE : EPISODE_WORKGROUP;
}

// dw_run_episode_mlp, once current and previous state are quantised (until then: launches per step whatever the form);
// *lds_bytes: the dynamic LDS of the launch
static EpisodeForm episode_mlp_form(const dw_handle* h, size_t* lds_bytes) {
    const dw_params& p = h->prm;
    const int Cc = p.height * p.width, N = p.n_agents;
    const int wpb = worlds_per_block(Cc);
    // H*W <= 256 with at most four agents (the ES trainers' own 16x16 x 4): one wave per world (dw_episode_wave.hpp)
    const bool wave_kernel = Cc <= kEwMaxCells && 16 * N <= 64 && !h->sw.no_episode_wave;
    const size_t lds = wave_kernel ? episode_wave_shared_bytes() + episode_mlp_wave_world_bytes(Cc, N) * 4
                                   : episode_mlp_world_bytes(Cc, N) * wpb;
    if (lds_bytes) *lds_bytes = lds;
    const bool small = Cc <= 4096 && lds <= 160 * 1024 && p.precision != DW_PRECISION_F64 && p.collision_mode == 0 &&
                       !h->sw.no_episode_kernel;
    return !small ? EPISODE_STEPWISE : (wave_kernel ? EPISODE_WAVE : EPISODE_WORKGROUP);
}

static bool episode_kernel_applies(const dw_handle* h) { return episode_form(h) != EPISODE_STEPWISE && cur_quantised(h); }

// The agents' part of a step of the stepwise episode loop: the actions of policy_mode - or, `from_table`, the caller's
// slice `codes` [B*N] (-1 / -2: greedy / anti-greedy) - into h->action, then grazing (d_ok: the ok flags straight from it)
static int launch_policy(dw_handle* h, int policy_mode, bool from_table, const unsigned char* codes, unsigned char* d_ok = nullptr) {
    const size_t bn = (size_t)h->prm.batch * h->prm.n_agents;
    if (policy_mode == DW_POLICY_TABLE || from_table) {
        hipLaunchKernelGGL(actions_from_table, dim3((unsigned)((bn + 255) / 256)), dim3(256), 0, h->stream,
                           reinterpret_cast<const signed char*>(codes), (int)bn, h->action.get());
        if (int rc = launch_policy_greedy(h, 0, nullptr, 1)) return rc;
    } else if (policy_mode == DW_POLICY_ZEROS) {
        HIPCHK(hipMemsetAsync(h->action.get(), 0, sizeof(int) * bn, h->stream));
    } else if (int rc = launch_policy_greedy(h, policy_mode == DW_POLICY_ARGMIN ? 1 : 0, nullptr, 0)) {
        return rc;
    }
    HIPCHK(hipGetLastError());
    return launch_agents(h, h->action.get(), h->prm.batch, h->prm.n_agents, false, nullptr, nullptr, d_ok);
}

// What fill_episode_io fills, and the table and the flags of the steps from `t0` on.  The one-wave-per-world kernels (`wave`) take a null
// use_table / table where the caller gave none.
static EpisodeIO episode_io(const dw_handle* h, int policy_mode, const EpisodeStaging& S, size_t t0, bool wave, bool have_use_table,
                            bool have_table) {
    using R = EpisodeStaging;
    unsigned char* dev = h->ep_buf.get();
    EpisodeIO io{};
    fill_episode_io(io, h, S);
    io.use_table = wave && !have_use_table ? nullptr : dev + S.off[R::USE_TABLE] + t0;
    io.table = wave && !have_table ? nullptr : reinterpret_cast<const signed char*>(dev + S.off[R::TABLE] + t0 * S.bn);
    io.world_alive = dev + S.off[R::WORLD_ALIVE] + t0 * S.B;
    io.agent_ok = dev + S.off[R::AGENT_OK] + t0 * S.bn;
    io.action = (h->prm.n_agents > 0 && policy_mode != kPolicySkipAgents) ? h->action.get() : nullptr;
    return io;
}

// An episode for shapes without an LDS-resident kernel: the same K steps as K x (policy, dw_step) issued back-to-back on
// the handle's stream - policy kernel or table slice -> update_agents -> step kernel -> flags from the step's reductions
// (`trace`, dw_run_episode_trace: and episode_stats_row_pw, which copies them into row t of the records) - with no host
// round trip in between; one synchronisation at the end.  With `worlds` (dw_run_episode_ensemble; `sym`: for
// launch_forward_pw) the step is that per-world single step of dw_step_n_trace_ensemble, from rows that go up as in the
// trace calls (PwTable, the table chunks of plan_series without the test hook).  Fused step pairs only without either: the
// step-1 sums of a pair would have to include the patch kernel's corrections, and the pair kernels take one constant set.
// With `frames` (dw_run_episode_frames; the caller has allocated the ring and uploaded the selection): single steps as with
// `trace`; around every stride-th step FrameRun::before - launch_tile_temp on the current planes, between update_agents
// and the step kernel - and FrameRun::after - launch_tile_cover and frame_agents_pw behind it.
// With `temps` (dw_run_episode_trace_temperature; the caller has allocated the reduction's partials): between a step's
// update_agents and its step kernel, the statistics of the temperature field that step computes - temp_moments_pw on the
// current planes at L_schedule[t], or with `worlds` (dw_run_episode_ensemble_trace) at each world's float64 row of the
// step - into row t of the temperature block; single steps as with `trace`.
static int run_episode_stepwise(dw_handle* h, int32_t nsteps, const double* L_schedule, int policy_mode,
                                const uint8_t* use_table, const int8_t* table, uint32_t threshold_k, uint8_t* world_alive,
                                uint8_t* agent_ok, dw_world_stats* trace, WorldRows* worlds = nullptr, bool sym = false,
                                dw_temp_stats* temps = nullptr, FrameRun* frames = nullptr) {
    using R = EpisodeStaging;
    const dw_params& p = h->prm;
    const int N = p.n_agents, B = p.batch;
    const size_t K = (size_t)nsteps, Bz = (size_t)B, bn = Bz * N;
    const bool plain = !trace && !worlds && !temps && !frames;
    EpisodeRegions regions;
    regions.trace = trace != nullptr || temps != nullptr; regions.temps = temps != nullptr; regions.pairs = plain; regions.slack = 256;
    EpisodeBuffers E(h, EpisodeStaging(K, Bz, (size_t)N, regions));
    SeriesSchedule q;
    std::optional<PwTable> tab;
    if (worlds) {
        q = plan_series(SeriesSpec{nsteps, Bz, sizeof(StatsDev), 0, 0, false, false, true, false, L_schedule});   // (single steps, no hook)
        tab.emplace(h, PwLayout(Bz, q.trows));
    }
    if (int rc = E.alloc(false)) return rc;
    if (tab)
        if (int rc = tab->alloc("the per-world constants", {tab->item()})) return rc;
    SyncOnExit guard(h->stream);                              // `table`, the flag arrays and `trace` are the caller's
    if (int rc = E.upload(nullptr, 0, true, nullptr, table)) return rc;
    unsigned char* const d_tab = E.dev(R::TABLE);
    unsigned char* const d_wa = E.dev(R::WORLD_ALIVE);
    unsigned char* const d_ok = E.dev(R::AGENT_OK);
    unsigned char* const d_code = E.dev(R::CODE);
    StatsDev* const rows = E.dev<StatsDev>(R::TRACE);
    TempStatsDev* const trows = reinterpret_cast<TempStatsDev*>(h->ep_buf.get() + E.S.temps_off());
    const int nflag = B > (int)bn ? B : (int)bn;
    // (with per-world constants DW_POLICY_ZEROS wins over use_table, without them use_table wins: DESIGN.md 3.2j)
    const bool table_steps = use_table && !(worlds && policy_mode == DW_POLICY_ZEROS);
    auto from_table = [&](size_t t) { return policy_mode == DW_POLICY_TABLE || (table_steps && use_table[t]); };
    // Step pairs on wide grids (dw_agents_fused.hpp): policy_t, graze_t, ONE fused launch for forward_t and
    // forward_{t+1}, then the agents' step t+1 recomputed around the agents and patched into the result.
    // Needs no per-step world reductions (the caller passed world_alive == NULL); the last step of the
    // call stays an ordinary step, so the handle ends exactly as after K calls of dw_step.
    const bool may_pair = plain && h->plan.allow_fuse && bn && N <= kLookaheadMaxAgents && policy_mode != kPolicySkipAgents &&
                          !h->sw.no_agent_fuse;
    // With per-step world flags the fused launch also reduces what the flags of both steps need (STATS
    // variants: exact step-1 maximum, count of certain step-2 values above the threshold).
    unsigned int* pstats = (plain && world_alive) ? E.dev<unsigned int>(R::PAIR_STATS) : nullptr;
    // zeroed once: every agents_lookahead_patch launch leaves its world's words cleared for the next pair
    if (pstats && may_pair) HIPCHK(hipMemsetAsync(pstats, 0, sizeof(unsigned int) * 2 * B, h->stream));
    // action codes of a pair's second step when they come from no table: one byte value for the whole episode
    const int uniform_code = policy_mode == DW_POLICY_ZEROS ? 0 : (policy_mode == DW_POLICY_ARGMIN ? 0xFE : 0xFF);
    if (may_pair && policy_mode != DW_POLICY_TABLE) HIPCHK(hipMemsetAsync(d_code, uniform_code, bn, h->stream));
    // policy + update_agents of the step after a pair run inside that pair's patch kernel (phase E) while the chunk
    // continues: two launches per pair instead of four (DW_NO_AGENT_PREAPPLY: experiments)
    const bool no_preapply = h->sw.no_agent_preapply;
    bool pre_applied = false;
    size_t c = 0;                                               // (worlds) the table chunk that starts next
    for (size_t t = 0; t < K; ++t) {
        if (tab && (int)t == (c ? q.chunks[c - 1].end : 0)) {
            if (int rc = tab->next_chunk(q, c, L_schedule, *worlds)) return rc;
            ++c;
        }
        const bool pair = may_pair && cur_quantised(h) && K - t >= 3;
        if (pre_applied) {
            pre_applied = false;                             // step t's policy and grazing were done by the last patch
        } else if (bn && policy_mode != kPolicySkipAgents) {
            // a pair's first step: the agents' ok flags straight from the grazing kernel
            if (int rc = launch_policy(h, policy_mode, from_table(t), d_tab + t * bn, pair ? d_ok + t * bn : nullptr)) return rc;
        }
        if (pair) {
            const double L1 = L_schedule[t], L2 = L_schedule[t + 1];
            int rc = launch_forward_fused2(h, L1, L2, pstats, (float)threshold_k);   // pstats: zero (see above)
            if (rc) return rc;
            LookaheadArgs A;                                 // (codes: the caller's table slice, or the uniform byte)
            A.inL = h->L16[1 - h->cur].get(); A.inD = h->D16[1 - h->cur].get();
            A.outL = h->L16[h->cur].get(); A.outD = h->D16[h->cur].get();
            A.idx = h->idx.get(); A.st = h->st.get();
            A.code = reinterpret_cast<const signed char*>(from_table(t + 1) ? d_tab + (t + 1) * bn : d_code);
            A.agent_ok = d_ok + (t + 1) * bn;
            A.code_next = nullptr;
            A.agent_ok_next = nullptr;
            A.action_out = h->action.get();
            if (t + 2 < K && !no_preapply) {                   // the chunk continues with step t+2
                A.code_next = reinterpret_cast<const signed char*>(from_table(t + 2) ? d_tab + (t + 2) * bn : d_code);
                A.agent_ok_next = d_ok + (t + 2) * bn;
                pre_applied = true;
            }
            A.alive_t = pstats ? d_wa + t * Bz : nullptr;
            A.alive_t1 = pstats ? d_wa + (t + 1) * Bz : nullptr;
            A.pstats = pstats; A.thr = threshold_k;
            A.B = B; A.N = N; A.H = p.height; A.W = p.width; A.mask = p.obs_mask;
            A.agent_gamma = p.agent_gamma;
            A.P1 = derive_f32(p, L1); A.P2 = derive_f32(p, L2);
            A.P64 = make_f64(p, L1); A.La = L1; A.Lb = L2;
            if (p.precision == DW_PRECISION_EXACT)
                hipLaunchKernelGGL((agents_lookahead_patch<true>), dim3((unsigned)B), dim3(64), 0, h->stream, A);
            else
                hipLaunchKernelGGL((agents_lookahead_patch<false>), dim3((unsigned)B), dim3(64), 0, h->stream, A);
            HIPCHK(hipGetLastError());
            ++t;                                             // two steps done
            continue;
        }
        if (temps)                                              // (worlds: each world at its own float64 row of the step)
            if (int rc = tab ? launch_temp_moments(h, /*current=*/true, 0.0, tab->lay.p64(tab->dev(), q.row_of[t]), trows + t * Bz)
                             : launch_temp_moments(h, /*current=*/true, L_schedule[t], nullptr, trows + t * Bz)) return rc;
        const bool frame = frames && (t + 1) % (size_t)frames->stride == 0;
        if (frame)                                              // the tile means of the field this step computes
            if (int rc = frames->before(L_schedule[t])) return rc;
        if (tab) {
            const size_t tr = q.row_of[t];
            if (int rc = launch_forward_pw(h, tab->lay.p32(tab->dev(), tr), tab->lay.p64(tab->dev(), tr), tab->lay.fb(tab->dev()), sym, true)) return rc;
        } else if (int rc = launch_forward(h, L_schedule[t])) {
            return rc;
        }
        hipLaunchKernelGGL(episode_flags, dim3((unsigned)((nflag + 255) / 256)), dim3(256), 0, h->stream,
                           h->stats2[h->sp].get(), h->st.get(), B, N, threshold_k, d_wa + t * Bz, d_ok + t * bn);
        if (trace)
            hipLaunchKernelGGL(episode_stats_row_pw, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream,
                               h->stats2[h->sp].get(), B, rows + t * Bz);
        HIPCHK(hipGetLastError());
        if (frame)                                              // the cover it left and the agents on it
            if (int rc = frames->after()) return rc;
    }
    if (int rc = E.finish(world_alive, agent_ok, trace, temps)) return rc;
    guard.disarm();
    return DW_OK;
}

// What dw_run_episode and dw_run_episode_ensemble require of the handle and of their arguments
static int check_episode_call(const dw_handle* h, int32_t nsteps, int policy_mode, const uint8_t* use_table, const int8_t* table) {
    const dw_params& p = h->prm;
    NEED(nsteps >= 1 && nsteps <= 4096, DW_EINVAL, "nsteps must be in 1..4096");
    NEED(p.precision != DW_PRECISION_F64, DW_EINVAL, "dw_run_episode supports exact and fast precision");
    NEED(p.collision_mode == 0, DW_EINVAL, "collision_mode=1 is not implemented on the device");
    NEED(h->have_state, DW_ESTATE, "no state uploaded");
    NEED(p.n_agents == 0 || h->have_agents, DW_ESTATE, "no agents uploaded");
    NEED(cur_quantised(h), DW_ESTATE, "the current state is not quantised yet; take the first step with dw_step");
    NEED(policy_mode != DW_POLICY_TABLE || table, DW_EINVAL, "DW_POLICY_TABLE needs a table");
    if (use_table && !table)
        for (int t = 0; t < nsteps; ++t) NEED(!use_table[t], DW_EINVAL, "use_table set but no table given");
    return DW_OK;
}

// `trace` (dw_run_episode_trace): also the records of every step, [K][B]; the one-wave-per-world form takes
// episode_wave_stats_pw, every other form launches per step: no LDS workgroup kernel, the stated price of the records.
// `temps` (dw_run_episode_trace_temperature): also the temperature records of every step, [K][B], behind the records in
// the staging buffer; the same dispatch with episode_wave_temp_pw, which writes both.
static int run_episode_impl(dw_handle* h, int32_t nsteps, const double* L_schedule, int policy_mode,
                            const uint8_t* use_table, const int8_t* table, uint32_t threshold_k,
                            uint8_t* world_alive, uint8_t* agent_ok, dw_world_stats* trace, dw_temp_stats* temps) {
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    if (int rc = check_episode_call(h, nsteps, policy_mode, use_table, table)) return rc;
    const int C = p.height * p.width, N = p.n_agents, B = p.batch;
    const EpisodeForm form = episode_form(h);                  // (F64 / collision_mode 1 were rejected above)
    const bool records = trace || temps;
    if (form == EPISODE_STEPWISE || (records && form != EPISODE_WAVE)) {
        if (temps)                                              // the partials of temp_moments_pw (the rows live in the staging buffer)
            if (int rc = alloc_group(h, "the temperature reduction", {{h->temp_part, temp_part_bytes(h)}})) return rc;
        return run_episode_stepwise(h, nsteps, L_schedule, policy_mode, use_table, table, threshold_k, world_alive, agent_ok, trace,
                                    nullptr, false, temps);
    }
    const bool wave_kernel = form == EPISODE_WAVE;
    const int wpb = worlds_per_block(C);
    const size_t world_bytes = wave_kernel ? episode_wave_world_bytes(C, N) : episode_world_bytes(C, N);
    const size_t lds = temps ? episode_wave_temp_lds_bytes(C, N)      // (<= 64 KB for every shape of the form: static_assert there)
                     : trace ? episode_wave_stats_lds_bytes(C, N)
                             : world_bytes * wpb + (wave_kernel ? episode_wave_shared_bytes() : 0);
    NEED(lds <= 160 * 1024, DW_EINVAL, "too many agents for the LDS-resident episode kernel");
    const size_t K = (size_t)nsteps;
    EpisodeRegions regions;
    regions.rows = K; regions.use_table = true; regions.trace = records; regions.temps = temps != nullptr;
    EpisodeBuffers E(h, EpisodeStaging(K, (size_t)B, (size_t)N, regions));
    if (int rc = E.alloc(E.S.fits_image())) return rc;
    PhysF32* p32 = E.p32();
    for (size_t t = 0; t < K; ++t) p32[t] = derive_f32(p, L_schedule[t]);
    SyncOnExit guard(h->stream);                              // E's images and the caller's arrays
    if (int rc = E.upload(L_schedule, K, true, use_table, table)) return rc;
    StatsDev* stats = h->stats2[h->sp].get();
    // episode_wave ASSIGNS every world's whole record (its float64 count in `reserved`) and the counter record behind them:
    // nothing to clear; episode_small accumulates: cleared as before
    if (!wave_kernel) HIPCHK(hipMemsetAsync(stats, 0, sizeof(StatsDev) * (B + 1), h->stream));
    const EpisodeIO io = episode_io(h, policy_mode, E.S, 0, wave_kernel, use_table != nullptr, table && E.S.bn);
    const PhysF64 P64 = make_f64(p, L_schedule[0]);
    const dim3 grid((unsigned)((B + wpb - 1) / wpb));
    const bool ex = p.precision == DW_PRECISION_EXACT;
    if (temps) {
        auto kern = ex ? episode_wave_temp_pw<true> : episode_wave_temp_pw<false>;
        const EpisodeWaveTempArgs A{io, E.dev<StatsDev>(EpisodeStaging::TRACE),
                                    reinterpret_cast<TempStatsDev*>(h->ep_buf.get() + E.S.temps_off()), B, N, p.height, p.width, nsteps,
                                    policy_mode, p.obs_mask, threshold_k, p.agent_gamma, P64};
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, h->stream, A);
    } else if (trace) {
        auto kern = ex ? episode_wave_stats_pw<true> : episode_wave_stats_pw<false>;
        const EpisodeWaveStatsArgs A{io, E.dev<StatsDev>(EpisodeStaging::TRACE), B, N, p.height, p.width, nsteps,
                                     policy_mode, p.obs_mask, threshold_k, p.agent_gamma, P64};
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, h->stream, A);
    } else if (wave_kernel) {
        auto kern = ex ? episode_wave<true> : episode_wave<false>;
        if (int rc = set_lds_limit(h, kern, lds)) return rc;
        const EpisodeWaveArgs A{io, B, N, p.height, p.width, nsteps, policy_mode, p.obs_mask, threshold_k, p.agent_gamma, P64};
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, h->stream, A);
    } else {
        auto kern = ex ? episode_small<true> : episode_small<false>;
        if (int rc = set_lds_limit(h, kern, lds)) return rc;
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, h->stream, io, B, N, p.height, p.width, wpb, nsteps, policy_mode,
                           p.obs_mask, p.agent_gamma, threshold_k, P64);
    }
    HIPCHK(hipGetLastError());
    episode_done(h, L_schedule[K - 1], false);
    release_unquantised(h);
    if (int rc = E.finish(world_alive, agent_ok, trace, temps)) return rc;      // flags are returned
    guard.disarm();
    return DW_OK;
}

// ---- dw_run_episode_trace: dw_run_episode with the records of every step ------------------------------------------
// The form the call takes: one wave per world (episode_wave_stats_pw) wherever dw_run_episode takes episode_wave; every
// other shape, DW_NO_EPISODE_WAVE and DW_NO_EPISODE_KERNEL: launches per step
int dw_run_episode_trace(dw_handle* h, int32_t nsteps, const double* L_schedule, int policy_mode,
                         const uint8_t* use_table, const int8_t* table, uint32_t threshold_k, uint8_t* world_alive,
                         uint8_t* agent_ok, dw_world_stats* trace) {
    NEED(h && L_schedule, DW_EINVAL, "null argument");
    NEED(trace, DW_EINVAL, "dw_run_episode_trace needs a trace array");
    NEED(policy_mode >= 0 && policy_mode <= 3, DW_EINVAL, "bad policy mode");
    return run_episode_impl(h, nsteps, L_schedule, policy_mode, use_table, table, threshold_k, world_alive, agent_ok, trace);
}

// ---- dw_run_episode_trace_temperature: dw_run_episode_trace with the temperature records of every step -----------------
// The form the call takes is dw_run_episode_trace's: one wave per world (episode_wave_temp_pw), or launches per step with
// temp_moments_pw in front of every step kernel.  Both reduce in temp_moments_pw's order: the same bytes.
int dw_run_episode_trace_temperature(dw_handle* h, int32_t nsteps, const double* L_schedule, int policy_mode,
                                     const uint8_t* use_table, const int8_t* table, uint32_t threshold_k, uint8_t* world_alive,
                                     uint8_t* agent_ok, dw_world_stats* trace, dw_temp_stats* temps) {
    NEED(h && L_schedule, DW_EINVAL, "null argument");
    NEED(temps, DW_EINVAL, "dw_run_episode_trace_temperature needs a temps array");
    NEED(policy_mode >= 0 && policy_mode <= 3, DW_EINVAL, "bad policy mode");
    static_assert(sizeof(dw_temp_stats) == sizeof(TempStatsDev) && sizeof(TempStatsDev) == EpisodeStaging::kTempRow, "temperature record layout");
    return run_episode_impl(h, nsteps, L_schedule, policy_mode, use_table, table, threshold_k, world_alive, agent_ok, trace, temps);
}

// ---- dw_run_episode_ensemble: dw_run_episode with a set of physics constants and a luminosity column per world --------
// The form the call takes: one wave per world (episode_wave_pw) wherever dw_run_episode takes episode_wave; every other
// shape, DW_NO_EPISODE_WAVE and DW_NO_EPISODE_KERNEL: launches per step, no LDS workgroup kernel.
// `records` (dw_run_episode_ensemble_trace): also the records of every step (`trace`) and the temperature records
// (`temps`), [K][B] each, either may be null; the same dispatch with episode_wave_ens_trace_pw<EXACT, temps given>, which
// always writes the cover records on the device, or the launches per step with the rows of the per-world table.
static int run_episode_ensemble_impl(dw_handle* h, int32_t nsteps, const dw_world_params* worlds, const double* L_schedule,
                                     int policy_mode, const uint8_t* use_table, const int8_t* table, uint32_t threshold_k,
                                     uint8_t* world_alive, uint8_t* agent_ok, bool records, dw_world_stats* trace,
                                     dw_temp_stats* temps) {
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    // every check before anything is launched or allocated: the rules of dw_run_episode, of the per-world schedules, and
    // of dw_set_params for each world's set
    if (int rc = check_episode_call(h, nsteps, policy_mode, use_table, table)) return rc;
    const int C = p.height * p.width, N = p.n_agents, B = p.batch;
    const size_t K = (size_t)nsteps, Bz = (size_t)B;
    const bool wave = episode_form(h) == EPISODE_WAVE;
    WorldRows rows_of(p, worlds, Bz, !wave);
    if (int rc = check_per_world(rows_of, worlds, L_schedule, K, Bz)) return rc;
    if (!wave) {
        if (temps)                                              // the partials of temp_moments_pw (the rows live in the staging buffer)
            if (int rc = alloc_group(h, "the temperature reduction", {{h->temp_part, temp_part_bytes(h)}})) return rc;
        return run_episode_stepwise(h, nsteps, L_schedule, policy_mode, use_table, table, threshold_k, world_alive, agent_ok, trace,
                                    &rows_of, worlds_symmetric(worlds, Bz) && !h->sw.no_sym, temps);
    }
    const size_t lds = records ? episode_wave_ens_trace_lds_bytes(C, N)
                               : episode_wave_pw_shared_bytes() + episode_wave_pw_world_bytes(C, N) * 4;
    NEED(lds <= 160 * 1024, DW_EINVAL, "too many agents for the LDS-resident episode kernel");
    // The kernel keeps a world in LDS for a whole launch; a call is one launch unless its table of rows (136 B per step and
    // world) would pass 32 MiB: then launches of `rows` steps (a multiple of the 64-step segment), each continuing from the
    // planes and agents the one before it wrote back - the same states, step for step - and writing its flags and records
    // from row t0 of their blocks on.
    const size_t row_bytes = (sizeof(PhysF32) + sizeof(double)) * Bz;
    size_t rows = ((size_t)32 << 20) / row_bytes / kEwSeg * kEwSeg;
    rows = rows < (size_t)kEwSeg ? (size_t)kEwSeg : rows;
    rows = rows > K ? K : rows;
    // staged: the first launch's inputs in ONE copy, a later launch's rows in one more, the call's flags (and records) in
    // one.  Flags only: always.  With records while the whole buffer fits the page-locked image (EpisodeStaging::fits_image);
    // beyond, the image holds the inputs alone and the outputs come down straight into the caller's arrays.
    EpisodeRegions regions;
    regions.rows = rows; regions.per_world = true; regions.use_table = true;
    regions.trace = records; regions.temps = records && temps != nullptr;
    EpisodeBuffers E(h, EpisodeStaging(K, Bz, (size_t)N, regions));
    if (int rc = E.alloc(true, records && !E.S.fits_image())) return rc;
    SyncOnExit guard(h->stream);                                // the image
    PhysF64* p64 = E.S.at<PhysF64>(E.img, EpisodeStaging::P64);
    for (size_t b = 0; b < Bz; ++b) p64[b] = make_f64(rows_of.params(b), 0.0);   // (L: replaced by the step's, from the Ls rows)
    const bool ex = p.precision == DW_PRECISION_EXACT;
    const dim3 grid((unsigned)((B + 3) / 4));
    auto plain_kern = ex ? episode_wave_pw<true> : episode_wave_pw<false>;
    auto rec_kern = temps ? (ex ? episode_wave_ens_trace_pw<true, true> : episode_wave_ens_trace_pw<false, true>)
                          : (ex ? episode_wave_ens_trace_pw<true, false> : episode_wave_ens_trace_pw<false, false>);
    if (int rc = records ? set_lds_limit(h, rec_kern, lds) : set_lds_limit(h, plain_kern, lds)) return rc;
    StatsDev* const d_trace = E.dev<StatsDev>(EpisodeStaging::TRACE);
    TempStatsDev* const d_temps = reinterpret_cast<TempStatsDev*>(h->ep_buf.get() + E.S.temps_off());
    PhysF32* r32 = E.p32();
    for (size_t t0 = 0; t0 < K; t0 += rows) {
        const size_t kk = K - t0 < rows ? K - t0 : rows;
        if (t0) HIPCHK(hipStreamSynchronize(h->stream));        // the image's rows are free again
        for (size_t t = 0; t < kk; ++t) rows_of.single(L_schedule + (t0 + t) * Bz, r32 + t * Bz, nullptr);
        if (int rc = E.upload(L_schedule + t0 * Bz, kk * Bz, t0 == 0, use_table, table)) return rc;
        // (every world's whole record is assigned by the kernel)
        const EpisodeIO io = episode_io(h, policy_mode, E.S, t0, true, use_table != nullptr, table && E.S.bn);
        if (records) {
            const EpisodeWaveEnsTraceArgs A{io, d_trace + t0 * Bz, temps ? d_temps + t0 * Bz : nullptr,
                                            E.dev<const PhysF64>(EpisodeStaging::P64), B, N, p.height, p.width, (int)kk, policy_mode,
                                            p.obs_mask, threshold_k, p.agent_gamma};
            hipLaunchKernelGGL(rec_kern, grid, dim3(256), lds, h->stream, A);
        } else {
            const EpisodeWavePwArgs A{io, E.dev<const PhysF64>(EpisodeStaging::P64), B, N, p.height, p.width, (int)kk, policy_mode,
                                      p.obs_mask, threshold_k, p.agent_gamma};
            hipLaunchKernelGGL(plain_kern, grid, dim3(256), lds, h->stream, A);
        }
        HIPCHK(hipGetLastError());
        episode_done(h, 0.0, true);
    }
    release_unquantised(h);
    if (int rc = E.finish(world_alive, agent_ok, trace, temps)) return rc;   // flags (and records) are returned
    guard.disarm();
    return DW_OK;
}

int dw_run_episode_ensemble(dw_handle* h, int32_t nsteps, const dw_world_params* worlds, const double* L_schedule, int policy_mode,
                            const uint8_t* use_table, const int8_t* table, uint32_t threshold_k, uint8_t* world_alive,
                            uint8_t* agent_ok) {
    NEED(h && worlds && L_schedule, DW_EINVAL, "null argument");
    NEED(policy_mode >= 0 && policy_mode <= 3, DW_EINVAL, "bad policy mode");
    return run_episode_ensemble_impl(h, nsteps, worlds, L_schedule, policy_mode, use_table, table, threshold_k, world_alive,
                                     agent_ok, false, nullptr, nullptr);
}

// ---- dw_run_episode_ensemble_trace: dw_run_episode_ensemble with the records of every step ------------------------------
// The form the call takes is dw_run_episode_ensemble's: one wave per world (episode_wave_ens_trace_pw), or launches per
// step with temp_moments_pw at the world's own float64 row in front of every step kernel.  Both reduce in
// temp_moments_pw's order: the same bytes.
int dw_run_episode_ensemble_trace(dw_handle* h, int32_t nsteps, const dw_world_params* worlds, const double* L_schedule,
                                  int policy_mode, const uint8_t* use_table, const int8_t* table, uint32_t threshold_k,
                                  uint8_t* world_alive, uint8_t* agent_ok, dw_world_stats* trace, dw_temp_stats* temps) {
    NEED(h && worlds && L_schedule, DW_EINVAL, "null argument");
    NEED(trace || temps, DW_EINVAL, "dw_run_episode_ensemble_trace needs a trace or a temps array (flags only: dw_run_episode_ensemble)");
    NEED(policy_mode >= 0 && policy_mode <= 3, DW_EINVAL, "bad policy mode");
    return run_episode_ensemble_impl(h, nsteps, worlds, L_schedule, policy_mode, use_table, table, threshold_k, world_alive,
                                     agent_ok, true, trace, temps);
}

// ---- dw_run_episode_frames: dw_run_episode_trace_temperature with frames of selected worlds ------------------------------
// One wave per world (episode_wave_frames_pw) wherever dw_run_episode_trace takes episode_wave_stats_pw: the call is split
// into launches at whole strides whose frames fit the ring (plan_frame_launches); the rows of every step go up once, a
// launch reads them from its first step on, and the ring comes down behind each launch by stream-ordered copies.
static int run_episode_frames_wave(dw_handle* h, int32_t nsteps, const double* L_schedule, int policy_mode, const uint8_t* use_table,
                                   const int8_t* table, uint32_t threshold_k, uint8_t* world_alive, uint8_t* agent_ok,
                                   dw_world_stats* trace, dw_temp_stats* temps, FrameRun& fr, const int* d_slot_of) {
    const dw_params& p = h->prm;
    const int C = p.height * p.width, N = p.n_agents, B = p.batch;
    const size_t K = (size_t)nsteps;
    const size_t lds = episode_wave_frames_lds_bytes(C, N);     // (<= 64 KB for every shape of the form: static_assert there)
    EpisodeRegions regions;
    regions.rows = K; regions.use_table = true; regions.trace = true; regions.temps = temps != nullptr;   // (the kernel always writes the records)
    EpisodeBuffers E(h, EpisodeStaging(K, (size_t)B, (size_t)N, regions));
    if (int rc = E.alloc(E.S.fits_image())) return rc;
    PhysF32* p32 = E.p32();
    for (size_t t = 0; t < K; ++t) p32[t] = derive_f32(p, L_schedule[t]);
    SyncOnExit guard(h->stream);                              // E's images and the caller's arrays
    if (int rc = E.upload(L_schedule, K, true, use_table, table)) return rc;
    const PhysF64 P64 = make_f64(p, L_schedule[0]);
    const dim3 grid((unsigned)((B + 3) / 4));
    const bool ex = p.precision == DW_PRECISION_EXACT;
    const int field = temps ? 2 : (fr.temp ? 1 : 0);
    const TileGeom& G = fr.sh.G;
    const EwFrameOut F{d_slot_of, fr.cover ? h->frame_cover.get() : nullptr, fr.temp ? h->frame_temp.get() : nullptr,
                       fr.agents ? h->frame_agents.get() : nullptr, fr.sh.S, fr.stride, G.th, G.tw, G.TW, (int)fr.sh.tiles, fr.sh.map};
    for (const FrameLaunch& l : plan_frame_launches(K, (size_t)fr.stride, fr.cap)) {
        EpisodeIO io = episode_io(h, policy_mode, E.S, l.t0, true, use_table != nullptr, table && E.S.bn);
        io.P32 += l.t0;                                         // (the rows of the whole call are on the device)
        io.Ls += l.t0;
        const EpisodeWaveFramesArgs A{io, E.dev<StatsDev>(EpisodeStaging::TRACE) + l.t0 * (size_t)B,
                                      temps ? reinterpret_cast<TempStatsDev*>(h->ep_buf.get() + E.S.temps_off()) + l.t0 * (size_t)B : nullptr,
                                      F, B, N, p.height, p.width, (int)l.steps, policy_mode, p.obs_mask, threshold_k, p.agent_gamma, P64};
        with_bool(ex, [&](auto EX) {
            with_int<0, 1, 2>(field, [&](auto FIELD) {
                hipLaunchKernelGGL((episode_wave_frames_pw<EX, FIELD>), grid, dim3(256), lds, h->stream, A);
            });
        });
        HIPCHK(hipGetLastError());
        episode_done(h, L_schedule[l.t0 + l.steps - 1], false);
        if (int rc = fr.download(l.f0, l.frames)) return rc;
    }
    release_unquantised(h);
    if (int rc = E.finish(world_alive, agent_ok, trace, temps)) return rc;      // flags and records are returned
    guard.disarm();
    return DW_OK;
}

int dw_run_episode_frames(dw_handle* h, int32_t nsteps, const double* L_schedule, int policy_mode, const uint8_t* use_table,
                          const int8_t* table, uint32_t threshold_k, uint8_t* world_alive, uint8_t* agent_ok, dw_world_stats* trace,
                          dw_temp_stats* temps, const dw_frame_spec* spec, int32_t stride, dw_tile_cover* cover, double* temp_mean,
                          dw_agent_frame* agents) {
    static_assert(sizeof(dw_agent_frame) == 16 && sizeof(dw_agent_frame) == sizeof(AgentFrameDev), "agent frame record layout");
    NEED(h && L_schedule && spec, DW_EINVAL, "null argument");
    NEED(policy_mode >= 0 && policy_mode <= 3, DW_EINVAL, "bad policy mode");
    NEED(stride >= 1, DW_EINVAL, "stride < 1");
    NEED(cover || temp_mean || agents, DW_EINVAL, "none of cover, temp_mean and agents is wanted (records only: dw_run_episode_trace*)");
    const dw_params& p = h->prm;
    NEED(!agents || p.n_agents > 0, DW_EINVAL, "agents are wanted of a handle without agents");
    HIPCHK(hipSetDevice(p.device));
    if (int rc = check_episode_call(h, nsteps, policy_mode, use_table, table)) return rc;
    FrameRun fr{h, FrameShape{}, stride, cover, temp_mean, agents};
    if (int rc = check_frame_spec(h, spec, &fr.sh)) return rc;
    fr.plan((size_t)(nsteps / stride));
    const bool wave = episode_form(h) == EPISODE_WAVE;
    // on the device: the selection [S] (a listed one) for the launches per step; for the waves every world's place in it [B]
    const size_t B = (size_t)p.batch;
    std::vector<int> slot_of(wave ? B : 0, -1);
    for (size_t s = 0; wave && s < (size_t)fr.sh.S; ++s) slot_of[fr.sh.listed ? (size_t)fr.sh.worlds[s] : s] = (int)s;
    if (int rc = alloc_group(h, "the frame buffers", {{h->frame_sel, wave ? sizeof(int) * B : fr.sh.sel_bytes()},
                                                       {h->frame_cover, fr.cover_bytes()}, {h->frame_temp, fr.temp_bytes()},
                                                       {h->frame_agents, fr.agents_bytes()},
                                                       {h->tile_part, !wave && temp_mean ? fr.sh.part_bytes() : 0},
                                                       {h->temp_part, !wave && temps ? temp_part_bytes(h) : 0}})) return rc;
    SyncOnExit sync(h->stream);                                 // the selection comes from the caller's array, the map from slot_of
    int rc;
    if (wave) {
        HIPCHK(hipMemcpyAsync(h->frame_sel.get(), slot_of.data(), sizeof(int) * B, hipMemcpyHostToDevice, h->stream));
        rc = run_episode_frames_wave(h, nsteps, L_schedule, policy_mode, use_table, table, threshold_k, world_alive, agent_ok, trace,
                                     temps, fr, h->frame_sel.get());
    } else {
        if ((rc = upload_selection(h, fr.sh))) return rc;
        rc = run_episode_stepwise(h, nsteps, L_schedule, policy_mode, use_table, table, threshold_k, world_alive, agent_ok, trace,
                                  nullptr, false, temps, &fr);
    }
    if (!rc) sync.disarm();                                     // (either form has synchronised)
    return rc;
}

// ---- device-side snapshots of the current state ----------------------------------------------------
// All regions of a snapshot in ONE launch (seven device-to-device copies were seven stream operations: ~55 us in front of
// every chunk of the fitness harness, whose whole chunk kernel takes 0.5 ms)
struct CopyJobs {
    const void* src[8];
    void* dst[8];
    unsigned long long bytes[8];
    int n;
};
__global__ __launch_bounds__(256) void copy_regions(CopyJobs J) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int j = 0; j < J.n; ++j) {
        const size_t nb = J.bytes[j];
        // (every region starts at the start of a device allocation: 256-byte aligned)
        const uint4* s16 = static_cast<const uint4*>(J.src[j]);
        uint4* d16 = static_cast<uint4*>(J.dst[j]);
        for (size_t i = t0; i < nb / 16; i += stride) d16[i] = s16[i];
        const unsigned char* s1 = static_cast<const unsigned char*>(J.src[j]);
        unsigned char* d1 = static_cast<unsigned char*>(J.dst[j]);
        for (size_t i = (nb & ~(size_t)15) + t0; i < nb; i += stride) d1[i] = s1[i];      // the last < 16 bytes
    }
}
static int launch_copy_regions(dw_handle* h, const CopyJobs& J) {
    size_t most = 0;
    for (int j = 0; j < J.n; ++j) {
        NEED(J.src[j] && J.dst[j], DW_EINVAL, "snapshot region not allocated");
        NEED(((reinterpret_cast<uintptr_t>(J.src[j]) | reinterpret_cast<uintptr_t>(J.dst[j])) & 15) == 0, DW_EINVAL,
             "snapshot region not 16-byte aligned");
        most = J.bytes[j] > most ? J.bytes[j] : most;
    }
    if (J.n == 0 || most == 0) return DW_OK;
    size_t blocks = (most / 16 + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks);
    hipLaunchKernelGGL(copy_regions, dim3((unsigned)blocks), dim3(256), 0, h->stream, J);
    HIPCHK(hipGetLastError());
    return DW_OK;
}

int dw_snapshot_save_slot(dw_handle* h, int32_t slot) {
    NEED(h, DW_EINVAL, "null handle");
    NEED(slot >= 0 && slot < DW_SNAPSHOT_SLOTS, DW_EINVAL, "snapshot slot out of range");
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    NEED(h->have_state, DW_ESTATE, "no state uploaded");
    NEED(cur_quantised(h), DW_ESTATE, "the current state is an un-quantised upload; take a step first");
    dw_handle::Snapshot& sn = h->snap[slot];
    sn.valid = false;                           // until the copy below is queued
    const size_t bn = (size_t)p.batch * p.n_agents;
    const size_t pb = sizeof(plane_t) * h->cells;
    const int rc = bn ? alloc_group(h, "a snapshot", {{sn.L, pb}, {sn.D, pb}, {sn.stats, h->stats_bytes},
                                                      {sn.idx, sizeof(int) * 2 * bn}, {sn.st, sizeof(double) * bn}})
                      : alloc_group(h, "a snapshot", {{sn.L, pb}, {sn.D, pb}, {sn.stats, h->stats_bytes}});
    if (rc) return rc;
    // the previous state too: observations (temperature channels) and the temp / beta / growth caches are
    // derived from it, so a replay from the snapshot must see the same one.  An un-quantised previous state
    // (the step after an upload) stays where it is: its buffers are not reused before the next upload, which
    // invalidates the snapshot.
    const bool keep_prev = h->stepped && h->unq != OWN_PREV;
    if (keep_prev)
        if (int prc = alloc_group(h, "a snapshot's previous state", {{sn.PL, pb}, {sn.PD, pb}})) return prc;
    CopyJobs J;
    J.n = 0;
    auto job = [&J](void* dst, const void* src, size_t bytes) { J.dst[J.n] = dst; J.src[J.n] = src; J.bytes[J.n] = bytes; ++J.n; };
    job(sn.L.get(), h->L16[h->cur].get(), pb);
    job(sn.D.get(), h->D16[h->cur].get(), pb);
    job(sn.stats.get(), h->stats2[h->sp].get(), h->stats_bytes);
    if (keep_prev) {
        job(sn.PL.get(), h->L16[1 - h->cur].get(), pb);
        job(sn.PD.get(), h->D16[1 - h->cur].get(), pb);
    }
    sn.stepped = h->stepped;
    sn.L_last = h->L_last;
    sn.L_per_world = h->L_per_world;
    sn.P_per_world = h->P_per_world;
    sn.unq = h->unq;
    sn.agents = bn && h->have_agents;
    if (sn.agents) {
        job(sn.idx.get(), h->idx.get(), sizeof(int) * 2 * bn);
        job(sn.st.get(), h->st.get(), sizeof(double) * bn);
    }
    if (int crc = launch_copy_regions(h, J)) return crc;
    sn.valid = true;
    return DW_OK;
}

int dw_snapshot_restore_slot(dw_handle* h, int32_t slot) {
    NEED(h, DW_EINVAL, "null handle");
    NEED(slot >= 0 && slot < DW_SNAPSHOT_SLOTS, DW_EINVAL, "snapshot slot out of range");
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    const dw_handle::Snapshot& sn = h->snap[slot];
    NEED(sn.valid, DW_ESTATE, "no snapshot saved in this slot (or a later upload / dw_init_random invalidated it)");
    const size_t bn = (size_t)p.batch * p.n_agents;
    const size_t pb = sizeof(plane_t) * h->cells;
    CopyJobs J;
    J.n = 0;
    auto job = [&J](void* dst, const void* src, size_t bytes) { J.dst[J.n] = dst; J.src[J.n] = src; J.bytes[J.n] = bytes; ++J.n; };
    job(h->L16[h->cur].get(), sn.L.get(), pb);
    job(h->D16[h->cur].get(), sn.D.get(), pb);
    job(h->stats2[h->sp].get(), sn.stats.get(), h->stats_bytes);
    if (sn.agents) {
        job(h->idx.get(), sn.idx.get(), sizeof(int) * 2 * bn);
        job(h->st.get(), sn.st.get(), sizeof(double) * bn);
    }
    if (sn.stepped && sn.unq != OWN_PREV) {
        job(h->L16[1 - h->cur].get(), sn.PL.get(), pb);
        job(h->D16[1 - h->cur].get(), sn.PD.get(), pb);
    }
    if (int rc = launch_copy_regions(h, J)) return rc;
    HIPCHK(hipMemsetAsync(h->stats2[1 - h->sp].get(), 0, h->stats_bytes, h->stream));
    h->unq = sn.unq;                            // OWN_PREV: the un-quantised initial state is still in its buffers
    h->stepped = sn.stepped;
    h->L_last = sn.L_last;
    h->L_per_world = sn.L_per_world;
    h->P_per_world = sn.P_per_world;
    return DW_OK;
}

int dw_snapshot_save(dw_handle* h) { return dw_snapshot_save_slot(h, 0); }
int dw_snapshot_restore(dw_handle* h) { return dw_snapshot_restore_slot(h, 0); }

// ---- plumbing ---------------------------------------------------------------------------------

int dw_set_stream(dw_handle* h, void* hip_stream) {
    NEED(h, DW_EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->prm.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->own_stream) HIPCHK(hipStreamDestroy(h->stream));
    h->stream = reinterpret_cast<hipStream_t>(hip_stream);
    h->own_stream = false;
    return DW_OK;
}

int dw_sync(dw_handle* h) {
    NEED(h, DW_EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->prm.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    return DW_OK;
}

int dw_timer_start(dw_handle* h) {
    NEED(h, DW_EINVAL, "null handle");
    HIPCHK(hipSetDevice(h->prm.device));
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    return DW_OK;
}

int dw_timer_stop(dw_handle* h, float* elapsed_ms) {
    NEED(h && elapsed_ms, DW_EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->prm.device));
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipEventSynchronize(h->ev1));
    HIPCHK(hipEventElapsedTime(elapsed_ms, h->ev0, h->ev1));
    return DW_OK;
}

int dw_device_planes(dw_handle* h, int which, void** light, void** dark) {
    NEED(h && light && dark, DW_EINVAL, "null argument");
    NEED(which == DW_STATE_CURRENT || which == DW_STATE_PREVIOUS, DW_EINVAL, "bad state selector");
    const int buf = which == DW_STATE_CURRENT ? h->cur : 1 - h->cur;
    NEED(which != DW_STATE_CURRENT || cur_quantised(h), DW_ESTATE,
         "the current state is an un-quantised upload: it has no binary16 planes before the first step");
    *light = h->L16[buf].get();
    *dark = h->D16[buf].get();
    return DW_OK;
}

int dw_kernel_info(dw_handle* h, char* buf, size_t buflen) {
    NEED(h && buf && buflen, DW_EINVAL, "null argument");
    const dw_params& p = h->prm;
    const StepPlan& pl = h->plan;
    const char* prec = p.precision == DW_PRECISION_EXACT ? "exact" : (p.precision == DW_PRECISION_FAST ? "fast" : "f64");
    static const char* const halo_name[] = {"rotate", "dpp-old", "general", "packed"};     // by halo_form
    if (pl.kind == STEP_STREAM) {
        const StripGeom& g = pl.sgeom;
        snprintf(buf, buflen,
                 "step_stream_%s<halo=%s> wave-strip=%dx256 cells, register window + DPP neighbours, %d-row blocks in "
                 "flight%s, %d strips, grid=%d x 256 threads (4 strips each), XCD-chunked",
                 prec, halo_name[pl.halo], g.SR,
                 p.precision == DW_PRECISION_EXACT ? DW_STREAM_RB_EXACT : DW_STREAM_RB_FAST,
                 p.precision == DW_PRECISION_EXACT ? ", in-wave float64 fix-up from an LDS queue" : "", g.nstrips,
                 g.chunk * 8);
        if (pl.allow_fuse) {
            const size_t n = std::strlen(buf);
            snprintf(buf + n, buflen - n, "; dw_step_n fuses step pairs (step_stream_fused2%s%s",
                     p.precision == DW_PRECISION_EXACT ? "_exact" : "",
                     pl.seam_strips ? "_seam_pw, format buffer accesses" : (pl.fmt_planes ? "_fmt_pw, format buffer accesses" : ""));
            if (pl.seam_strips) {
                const size_t m = std::strlen(buf);
                snprintf(buf + m, buflen - m, ", seam strips: %d x %d columns + %d columns of %d row bands per wave", pl.seam_geom.ncs,
                         kSeamCols, pl.left_geom.cols_per_strip, pl.left_geom.wpr);
            }
            if (pl.row_landing) {
                const size_t m = std::strlen(buf);
                snprintf(buf + m, buflen - m, ", rows land in place: step_stream_fused2_land_seam_pw + _land_left_pw");
            }
            const size_t m = std::strlen(buf);
            snprintf(buf + m, buflen - m, ")");
        }
    } else if (pl.kind == STEP_TILED) {
        const int TR = (256 / pl.tcq) * pl.rpt;
        snprintf(buf, buflen,
                 "step_tiled<TCQ=%d,RPT=%d,%s> tile=%dx%d cells, %zu B LDS/workgroup, %d tiles, grid=%d x 256 threads, "
                 "XCD-chunked",
                 pl.tcq, pl.rpt, prec, TR, pl.tcq * 4, pl.tile_lds, pl.geom.ntiles, pl.geom.chunk * 8);
    } else {
        snprintf(buf, buflen, "step_generic<%s> one thread per cell, grid=(%d,%d) x 256 threads", prec,
                 (p.height * p.width + 255) / 256, p.batch);
    }
    {                                                           // the form dw_step_n_trace takes (StepPlan::trace_pairs)
        const size_t n = std::strlen(buf);
        snprintf(buf + n, buflen - n, pl.trace_pairs ? "; trace: step pairs" : "; trace: single steps");
    }
    {                                                           // the form dw_step_n_trace_per_world takes (StepPlan::pw_stream)
        const size_t n = std::strlen(buf);
        snprintf(buf + n, buflen - n, pl.pw_stream ? "; per-world L: wave strips" : "; per-world L: generic");
    }
    {                                                           // the forms dw_run_episode / dw_run_episode_mlp take
        static const char* const form_name[] = {"launches per step", "workgroup (LDS)", "one wave per world"};   // by EpisodeForm
        const size_t n = std::strlen(buf);
        snprintf(buf + n, buflen - n, "; episode: %s; mlp episode: %s", form_name[episode_form(h)], form_name[episode_mlp_form(h)]);
    }
    {                                                           // the form dw_run_episode_ensemble takes
        const size_t n = std::strlen(buf);
        snprintf(buf + n, buflen - n, "; ensemble episode: %s", episode_form(h) == EPISODE_WAVE ? "one wave per world" : "launches per step");
    }
    {                                                           // the form dw_run_episode_trace takes
        const size_t n = std::strlen(buf);
        snprintf(buf + n, buflen - n, "; episode trace: %s", episode_form(h) == EPISODE_WAVE ? "one wave per world" : "launches per step");
    }
    {                                                           // the form dw_run_episode_trace_temperature takes
        const size_t n = std::strlen(buf);
        snprintf(buf + n, buflen - n, "; episode temperature: %s", episode_form(h) == EPISODE_WAVE ? "one wave per world" : "launches per step");
    }
    {                                                           // the form dw_run_episode_ensemble_trace takes
        const size_t n = std::strlen(buf);
        snprintf(buf + n, buflen - n, "; ensemble trace: %s", episode_form(h) == EPISODE_WAVE ? "one wave per world" : "launches per step");
    }
    {                                                           // the form dw_run_episode_mlp_trace takes
        const size_t n = std::strlen(buf);
        snprintf(buf + n, buflen - n, "; mlp trace: %s", episode_mlp_form(h) == EPISODE_WAVE ? "one wave per world" : "launches per step");
    }
    {                                                           // the form dw_run_episode_frames takes
        const size_t n = std::strlen(buf);
        snprintf(buf + n, buflen - n, "; episode frames: %s", episode_form(h) == EPISODE_WAVE ? "one wave per world" : "launches per step");
    }
    {                                                           // the form dw_run_episode_mlp_counts takes
        const size_t n = std::strlen(buf);
        snprintf(buf + n, buflen - n, "; mlp counts: %s", episode_mlp_counts_workgroup(h) ? "workgroup (LDS)" : "launches per step");
    }
    if (pl.first_stream) {                                      // the first step's wave-strips have a height of their own
        const size_t n = std::strlen(buf);
        snprintf(buf + n, buflen - n, "; first step: wave-strip=%dx256", pl.first_geom.SR);
    }
    if (h->sw.text[0]) {                                        // the switches this handle was created under
        const size_t n = std::strlen(buf);
        snprintf(buf + n, buflen - n, "; switches[%s]", h->sw.text);
    }
    {                                                           // the form dw_step_n_trace_ensemble takes (trace_per_world)
        const size_t n = std::strlen(buf);
        snprintf(buf + n, buflen - n, "; per-world constants: %s",
                 ensemble_pairs(h) ? "step pairs" : (pl.pw_stream ? "wave strips" : "generic"));
    }
    return DW_OK;
}

int dw_audit_tie_bound(dw_handle* h, double L, double out[4]) {
    NEED(h && out, DW_EINVAL, "null argument");
    const dw_params& p = h->prm;
    HIPCHK(hipSetDevice(p.device));
    NEED(h->have_state && cur_quantised(h), DW_ESTATE, "the audit needs a quantised current state");
    const StepPlan& pl = h->plan;
    int rc = ensure_scratch(h, 4 * sizeof(unsigned long long));
    if (rc) return rc;
    unsigned long long* d = reinterpret_cast<unsigned long long*>(h->scratch.get());
    HIPCHK(hipMemsetAsync(d, 0, 4 * sizeof(unsigned long long), h->stream));
    for_world_slices(p.batch, [&](int b0, int nb) {
        const dim3 g((unsigned)((p.height * p.width + 255) / 256), (unsigned)nb);
        const size_t w = (size_t)b0 * p.height * p.width;
        hipLaunchKernelGGL(tie_audit, g, dim3(256), 0, h->stream, h->L16[h->cur].get() + w, h->D16[h->cur].get() + w, p.height,
                           p.width, derive_f32(p, L), make_f64(p, L), d, pl.sym_albedo && pl.kind == STEP_STREAM ? 1 : 0);
    });
    HIPCHK(hipGetLastError());
    unsigned long long r[4];
    HIPCHK(hipMemcpyAsync(r, d, sizeof(r), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::memcpy(&out[0], &r[0], sizeof(double));
    std::memcpy(&out[1], &r[1], sizeof(double));
    out[2] = (double)r[2];
    out[3] = (double)r[3];
    return DW_OK;
}

int dw_last_fixup_count(dw_handle* h, uint64_t* count) {
    NEED(h && count, DW_EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->prm.device));
    // the counter behind the per-world records + the per-world counts of the one-wave-per-world episode kernels (`reserved`:
    // zero after every other kernel - the step kernels clear the whole buffer for the step after them)
    std::vector<StatsDev> st((size_t)h->prm.batch + 1);
    HIPCHK(hipMemcpyAsync(st.data(), h->stats2[h->sp].get(), sizeof(StatsDev) * st.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    unsigned long long v = st[h->prm.batch].sum_l;
    for (int b = 0; b < h->prm.batch; ++b) v += st[b].reserved;
    *count = v;
    return DW_OK;
}

}  // extern "C"
