// The opaque context behind the C ABI: packed weights, frame state, scratch arenas, counters.
#pragma once
#include "ra_kernels.hpp"
#include <memory>

struct HostNets {
    GeoNet geo{};
    MatNet mat{};
    ColNet col{};
    bool has_color = false;
    float beta = 0.1f;
    std::vector<uint16_t> sarena;      // K3 weight stream (consumption order, 1952 fragments of 1 KB), every layer padded; host only (prefix of fwd_arena)
    std::vector<uint16_t> sarena_trim; // the 8-wave K3's stream: sarena without the fragments that only hold padding (1920)
    std::vector<uint16_t> sarena_pairs;  // the same with the row blocks of every layer interleaved in pairs (K3 latency variants)
    std::vector<uint16_t> sarena_c;    // K3C: every fragment as an IEEE-half [hi | lo] pair in the 16x16x32 layout (3872 fragments), then K3CC's four per-wave streams (4 x 992)
    std::vector<uint16_t> fwd_arena;   // K4 forward stream: sarena + the 256 feature rows (2080 fragments)
    std::vector<uint16_t> bwd_arena;   // K4 backward stream: transposed geometry layers, then the material / colour head
    int bwd_geo_frags = 0, bwd_frags = 0;
    std::vector<float> shead_row;      // lin8 row 0 (sdf) in fp32: seed of the backward pass
    std::vector<float> barena;
    std::vector<float> cond_r0, b_r0, cond_r4, b_r4, cond_c3, b_c3;   // fp32 cond slices [256][cond]
    std::vector<float> light_xyz, light_area, light_sharp;
};

struct DevBuf {             // owns its device block: freed with the buffer (on the device that is current then); movable, not copyable
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); return *this; }
    ~DevBuf() { release(); }
    int ensure(size_t need);   // grow-only; returns non-zero on failure
    void release();
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// serialises the light-visibility stages of the contexts that share it (include/relightableavatar.h, "frames in flight")
struct ra_gate {
    int device = 0;
    hipEvent_t done = nullptr;      // end of the last stage submitted through the gate
    bool armed = false;
    ~ra_gate() { if (done) hipEventDestroy(done); }
};

// Pinned host staging for small per-frame inputs (bone poses): a slot is filled by the host, copied H2D asynchronously and may be refilled
// once its event has passed — the host never waits for the stream unless it runs more than `n` frames ahead.
struct PinRing {
    static constexpr int n = 8;
    char* base = nullptr;
    size_t slot_bytes = 0;
    int next = 0;
    hipEvent_t ev[n] = {};
    bool used[n] = {};
};

// Launch-variant hints.  The fused MLP kernels are persistent over tiles and correct for ANY device-side count; which variant (workgroup
// width) a launch gets only decides its speed, and it is chosen from a host-side UPPER BOUND of the count.  Where the bound is far above
// the real count (the ground pass: pixels x 512 lights against a handful of fine points), the 8-wave kernel ran almost empty.  Each render
// call therefore copies its fine-count slots to pinned memory behind an event when it ends, and the SAME call of a later frame (calls are
// numbered from ra_set_frame) reads them — if the event has passed; the host never waits — as a hint for the variant choice only.
struct HintSlot {
    hipEvent_t ev = nullptr;
    int* host = nullptr;        // pinned, HINT_SLOTS ints
    bool pending = false;
    int n_pending = 0;          // fine-count slots the pending copy holds
    int n_valid = 0;
    std::vector<int> vals;
};

// A triangle mesh built for closest-point queries (ra_mesh_create, ra_mesh.hip): owned by its context (ra_ctx::meshes), immutable once built
struct ra_mesh {
    MeshView view{};
    DevBuf recs, lbox, gbox;        // face records in leaf order, leaf boxes, group boxes
    std::vector<int> faces;         // the caller's face array: staging of the upload, alive as long as the copy may be pending
};

// The connectivity of a triangle mesh (ra_topo_create, ra_topo.hip): owned by its context (ra_ctx::topos), immutable once built.  The
// edge-sized arrays are allocated at their upper bound 3 n_faces, so that the build needs E only in its one read-back
struct ra_topo {
    TopoView view{};
    int max_nbr = 0, max_out = 0;       // the longest neighbour list and the most half-edges that leave one vertex
    int max_count = 0;                  // the most half-edges on one edge
    int readbacks = 0;                  // blocking read-backs of the build
    DevBuf vert, twin, edge, edges, counts, ehe_start, ehe, nbr_start, nbr, out_start, out_he;
    // the Loop coefficients (w_self, beta) of every outgoing count 0..max_out (ra_topo_rules.hpp: loop_weights); host copy = staging
    DevBuf loop_w;
    std::vector<float> loop_w_host;
};

// A garment on a topology (ra_cloth_create, ra_cloth.hip): owned by its context (ra_ctx::cloths), immutable once built.  It reads its
// topology's arrays, so the topology must outlive it.
struct ra_cloth {
    const ra_topo* topo = nullptr;
    double coeffs[5] = {};              // A, stretch_coeff, bending_coeff, lame_mu, lame_lambda (float64, host)
    float thickness = 0.f, mu = 0.f, lambda = 0.f, bending = 0.f;       // rounded once
    DevBuf frec, f_area, dm, dm_inv, hrec, h_faces, h_verts, mass, inv_mass, vh, vh_count;
};

// The size query of ra_marching_cubes / ra_mesh_largest_component that the next writing call completes: what it was asked and what it
// answered.  The offsets it computed stay in the context's scratch ("mc_*", "lcc_*") until then.
struct McQuery {
    const float* vol = nullptr;
    int nx = 0, ny = 0, nz = 0;
    float iso = 0.f;
    int n_verts = 0, n_faces = 0;
    int readbacks = 0;      // blocking read-backs of the last size query (ra_mesh_extract_stats)
    bool valid = false;
};
struct LccQuery {
    const float* verts = nullptr;
    const int* faces = nullptr;
    int n_verts = 0, n_faces = 0, out_verts = 0, out_faces = 0;
    int readbacks = 0, passes = 0;      // of the last size query: blocking read-backs, label passes that lowered a label (ra_mesh_extract_stats)
    bool valid = false;
};

// what a timed launch was (Timer, ra_get_kernel_time)
enum TimerKind { T_K3_WIDE = 0, T_K4 = 1, T_K3_NARROW = 2, T_K3C = 3 };      // 8-wave K3, full query (K4 pair), narrow K3, K3C

struct ra_ctx {
    int device = 0;
    std::vector<HintSlot> hints;    // per render call since ra_set_frame
    int call_no = 0;
    HintSlot* cur_hint = nullptr;
    PinRing pin;
    ra_gate* gate = nullptr;
    ra_config cfg{};
    bool have_cfg = false, have_weights = false, have_frame = false;
    bool k3cc_ok = true;        // K3CC's self-test against K3C at ra_finalize_weights (bit for bit); false -> launches of <= 8 Ki points use K3C's 4-wave tiles
    std::map<std::string, std::vector<float>> state_dict;
    std::vector<float> heads_theta;   // ra_heads_get_params: the material heads of state_dict in the flat layout (staging for the async copy)
    HostNets host;
    // device copies
    DevBuf sarena, sarena_pairs, sarena_c, fwd_arena, bwd_arena, shead_row, barena, cond_r0, cond_r4, cond_c3, b_r0, b_r4, b_c3, light_xyz, light_area, light_sharp, light_dir;
    int n_lights = 0;
    // light_xyz / light_dir are the positions every consumer reads: the loaded light_xyz_ unless ra_set_light_xyz moved them
    DevBuf light_xyz_loaded;      // light_xyz_ as loaded (ra_finalize_weights): what ra_set_light_xyz(NULL) copies back
    // the key-light tier (ra_config.key_light_share): per-light flags of the current frame's probes, on the device
    DevBuf key_mask, key_share;   // (key_share: every light's largest share of a probe's power among the frame's probes)
    bool key_valid = false;       // the flags were computed for the probes this frame is shaded with
    bool key_external = false;    // ... by ra_set_key_probes (the novel-light renderer: every probe of the re-shade); else per render call
    // LPIPS (ra_lpips_load): the packed AlexNet / lin weights; host copy = staging of the upload
    DevBuf lpips_arena;
    std::vector<float> lpips_host;
    bool lpips_loaded = false;
    // closest-point meshes still alive (ra_mesh_create); freed with the context
    std::vector<std::unique_ptr<ra_mesh>> meshes;
    // mesh connectivity still alive (ra_topo_create); freed with the context
    std::vector<std::unique_ptr<ra_topo>> topos;
    // garments still alive (ra_cloth_create); freed with the context
    std::vector<std::unique_ptr<ra_cloth>> cloths;
    // mesh extraction: the pending size queries (ra_marching_cubes, ra_mesh_largest_component)
    int vol_readbacks = 0;      // blocking read-backs of the last ra_sdf_volume
    McQuery mc_query;
    LccQuery lcc_query;
    // frame
    FrameState fr{};
    DevBuf fvertA, fpverts4, fbias_r0, fbias_r4, fbias_c3, fbvh_pts, fbvh_pairs, fbvh_order;
    bool use_bvh = true;
    // N3: vertex -> incident corners of the template mesh (built once per faces array)
    DevBuf adj_start, adj_list, adj_dfaces;
    unsigned long long adj_hash = 0;
    int adj_n_faces = 0, adj_n_verts = 0;
    // scratch (grow-only)
    std::map<std::string, DevBuf> scratch;
    DevBuf dcounters;       // DevCounters (64 B) + at byte 128: the int counters of a chunk (ra_api_impl.hpp: CNT_*; ra_api.cpp: the fine-count slots)
    int fc_next = 0;        // next unused fine-count slot (each hdq pass takes a fresh, still-zero one)
    bool fc_wrapped = false;
    bool cnt_zero = false;  // the named counters (hit / ray / sample counts) were zeroed by the chunk's bulk memset
    // host-side counters
    uint64_t n_shaded = 0;
    // timing of the fused MLP launches
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    std::vector<TimerKind> ev_kind;
    size_t ev_used = 0;

    ~ra_ctx();      // the events and pinned blocks of ev_pool, pin and hints; the DevBufs free themselves (ra_ctx_destroy makes the device current)

    template <typename T> T* buf(const std::string& name, size_t count, int* err) {
        DevBuf& b = scratch[name];
        if (b.ensure(count * sizeof(T))) { *err = 1; return nullptr; }
        return b.as<T>();
    }
};

int ra_pack_weights(ra_ctx* ctx, std::string& err);
