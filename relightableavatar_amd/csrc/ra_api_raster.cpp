// C ABI: the differentiable rasteriser — rasterisation and interpolation with their backwards (ra_raster.hip), antialiasing, the texture path
#include "ra_api_impl.hpp"
#include "ra_raster_rules.hpp"
#include "ra_antialias.hpp"
#include "ra_texture.hpp"

extern "C" {

int ra_raster_tile(int which) { return which == 0 ? RASTER_TILE : which == 1 ? RASTER_BLOCK : which == 2 ? RASTER_MAX_CHANNELS : 0; }

static bool raster_sizes_ok(int B, int H, int W) { return B >= 1 && H >= 1 && W >= 1 && (long long)B * H * W < (1ll << 31); }

int ra_rasterize(ra_ctx* c, const float* pos, int B, int V, const int* faces, int F, int H, int W, int flags, float* uv, float* zw, int* face,
                 void* stream) {
    // sizes and flags first: they need no ctx, so a caller's mistake is named before anything is dereferenced or launched
    RA_CHECK(raster_sizes_ok(B, H, W) && V >= 0 && V < (1 << 29) && F >= 0 && F < RASTER_MAX_FACES && (long long)B * F < (1ll << 31) - 1 && (V > 0 || F == 0),
             "ra_rasterize: bad sizes (B, H, W >= 1, B x H x W < 2^31, F < 2^24, B x F < 2^31; faces need vertices)");
    RA_CHECK((flags & ~RA_RASTER_BRUTE) == 0, "ra_rasterize: unknown flag");
    RA_CHECK(c && uv && zw && face, "ra_rasterize: null argument");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    const size_t n_pix = (size_t)B * H * W;
    if (F == 0) {               // empty maps: nothing is launched
        RA_HIP(hipMemsetAsync(uv, 0, n_pix * 2 * sizeof(float), s));
        RA_HIP(hipMemsetAsync(zw, 0, n_pix * sizeof(float), s));
        RA_HIP(hipMemsetAsync(face, 0xff, n_pix * sizeof(int), s));
        return 0;
    }
    RA_CHECK(pos && faces, "ra_rasterize: null argument (pos, faces)");
    const bool brute = (flags & RA_RASTER_BRUTE) != 0;
    const size_t n = (size_t)B * F;
    RasterJob j{};
    j.pos = pos; j.faces = faces; j.B = B; j.V = V; j.F = F; j.H = H; j.W = W; j.uv = uv; j.zw = zw; j.face = face;
    int err = 0;
    j.recs = c->buf<float4>("raster_recs", n * 5, &err);
    j.stat = c->buf<int>("raster_stat", 2, &err);
    if (!brute) {
        j.temp_bytes = raster_temp_bytes((long long)n + 1, 0);
        j.counts = c->buf<unsigned long long>("raster_counts", n + 1, &err);
        j.off = c->buf<unsigned long long>("raster_off", n + 1, &err);
        j.temp = c->buf<char>("raster_tmp", j.temp_bytes + 16, &err);
    }
    RA_CHECK(!err, "ra_rasterize: out of device memory");
    RA_HIP(hipMemsetAsync(j.stat, 0, 2 * sizeof(int), s));
    RA_CHECK(launch_raster_setup(j, s) == 0, "ra_rasterize: device scan failed");
    RA_HIP(hipGetLastError());
    int stat[2] = {};           // the one read-back: the (tile, face) pair count, which sizes the keys, and the face-index verdict
    RA_HIP(hipMemcpyAsync(stat, j.stat, sizeof(stat), hipMemcpyDeviceToHost, s));
    RA_HIP(hipStreamSynchronize(s));
    RA_CHECK(stat[1] == 0, "ra_rasterize: face index outside [0, n_verts)");
    long long n_pairs = -1;
    if (!brute) {
        n_pairs = stat[0];
        RA_CHECK(n_pairs < 0x7fffffff, "ra_rasterize: bad sizes (2^31 or more (tile, face) pairs)");
        j.temp_bytes = raster_temp_bytes(0, n_pairs);
        j.keys = c->buf<unsigned long long>("raster_keys", (size_t)n_pairs + 1, &err);
        j.keys_sorted = c->buf<unsigned long long>("raster_keys_sorted", (size_t)n_pairs + 1, &err);
        j.temp = c->buf<char>("raster_sort_tmp", j.temp_bytes + 16, &err);
        RA_CHECK(!err, "ra_rasterize: out of device memory");
    }
    RA_CHECK(launch_raster_tiles(j, n_pairs, s) == 0, "ra_rasterize: device sort failed");
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_interpolate(ra_ctx* c, const float* attr, int per_view, int V, int A, const int* faces, int F, const float* uv, const int* face, int B, int H, int W,
                   float* out, void* stream) {
    RA_CHECK(raster_sizes_ok(B, H, W) && V >= 0 && V < (1 << 29) && F >= 0 && F < RASTER_MAX_FACES && A >= 1 && A <= RASTER_MAX_CHANNELS &&
             (long long)B * V * A < (1ll << 40), "ra_interpolate: bad sizes (B, H, W >= 1, B x H x W < 2^31, F < 2^24, 1 <= A <= 64)");
    RA_CHECK(c && out, "ra_interpolate: null argument");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    if (F == 0 || V == 0) {
        RA_HIP(hipMemsetAsync(out, 0, (size_t)B * H * W * A * sizeof(float), s));
        return 0;
    }
    RA_CHECK(attr && faces && uv && face, "ra_interpolate: null argument (attr, faces, uv, face)");
    InterpJob j{};
    j.attr = attr; j.faces = faces; j.uv = uv; j.face = face; j.B = B; j.V = V; j.F = F; j.H = H; j.W = W; j.A = A; j.per_view = per_view != 0; j.out = out;
    launch_interpolate(j, s);
    RA_HIP(hipGetLastError());
    return 0;
}

// the pixels of every (view, face) in ascending order, for the two backward passes
static int raster_pixel_runs(ra_ctx* c, const int* face, int B, int F, int H, int W, unsigned long long** sorted, hipStream_t s) {
    const size_t n = (size_t)B * H * W;
    int err = 0;
    const size_t tb = raster_temp_bytes(0, (long long)n);
    unsigned long long* keys = c->buf<unsigned long long>("raster_pix_keys", n, &err);
    *sorted = c->buf<unsigned long long>("raster_pix_sorted", n, &err);
    void* temp = c->buf<char>("raster_sort_tmp", tb + 16, &err);
    if (err) return 1;
    return launch_raster_pixel_sort(face, B, F, H, W, keys, *sorted, temp, tb, s) ? 2 : 0;
}

int ra_interpolate_backward(ra_ctx* c, const ra_topo* topo, const float* attr, int per_view, int V, int A, const float* uv, const int* face, int B, int H,
                            int W, const float* dout, float* dattr, float* duv, void* stream) {
    RA_CHECK(raster_sizes_ok(B, H, W) && V >= 0 && A >= 1 && A <= RASTER_MAX_CHANNELS,
             "ra_interpolate_backward: bad sizes (B, H, W >= 1, B x H x W < 2^31, 1 <= A <= 64)");
    RA_CHECK(c && topo && (dattr || duv), "ra_interpolate_backward: null argument");
    RA_CHECK(owned(c->topos, topo), "ra_interpolate_backward: not a topology of this ctx");
    const TopoView& t = topo->view;
    RA_CHECK(raster_sizes_ok(B, H, W) && V == t.n_verts && t.n_faces < RASTER_MAX_FACES && A >= 1 && A <= RASTER_MAX_CHANNELS &&
             (long long)B * t.n_faces < (1ll << 31) - 1 && (long long)B * t.n_faces * 3 * A < (1ll << 40),
             "ra_interpolate_backward: bad sizes (B, H, W >= 1, B x H x W < 2^31, n_verts of the topology, F < 2^24, B x F < 2^31, 1 <= A <= 64)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    const size_t n_pix = (size_t)B * H * W;
    if (t.n_faces == 0 || V == 0) {
        if (dattr && V > 0) RA_HIP(hipMemsetAsync(dattr, 0, (size_t)(per_view ? B : 1) * V * A * sizeof(float), s));
        if (duv) RA_HIP(hipMemsetAsync(duv, 0, n_pix * 2 * sizeof(float), s));
        return 0;
    }
    RA_CHECK(attr && uv && face && dout, "ra_interpolate_backward: null argument (attr, uv, face, dout)");
    InterpJob j{};
    j.attr = attr; j.faces = t.vert; j.uv = uv; j.face = face; j.B = B; j.V = V; j.F = t.n_faces; j.H = H; j.W = W; j.A = A; j.per_view = per_view != 0;
    unsigned long long* sorted = nullptr;
    float* g_face = nullptr;
    if (dattr) {
        int err = 0;
        g_face = c->buf<float>("raster_g_face", (size_t)B * t.n_faces * 3 * A, &err);
        RA_CHECK(!err, "ra_interpolate_backward: out of device memory");
        const int rc = raster_pixel_runs(c, face, B, t.n_faces, H, W, &sorted, s);
        RA_CHECK(rc != 1, "ra_interpolate_backward: out of device memory");
        RA_CHECK(rc == 0, "ra_interpolate_backward: device sort failed");
    }
    launch_interpolate_backward(j, t, sorted, dout, g_face, dattr, duv, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_rasterize_backward(ra_ctx* c, const ra_topo* topo, const float* pos, int B, int V, int H, int W, const float* uv, const int* face, const float* duv,
                          float* dpos, void* stream) {
    RA_CHECK(raster_sizes_ok(B, H, W) && V >= 0, "ra_rasterize_backward: bad sizes (B, H, W >= 1, B x H x W < 2^31)");
    RA_CHECK(c && topo && dpos, "ra_rasterize_backward: null argument");
    RA_CHECK(owned(c->topos, topo), "ra_rasterize_backward: not a topology of this ctx");
    const TopoView& t = topo->view;
    RA_CHECK(raster_sizes_ok(B, H, W) && V == t.n_verts && V < (1 << 29) && t.n_faces < RASTER_MAX_FACES && (long long)B * t.n_faces < (1ll << 31) - 1,
             "ra_rasterize_backward: bad sizes (B, H, W >= 1, B x H x W < 2^31, n_verts of the topology, F < 2^24, B x F < 2^31)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    if (V == 0) return 0;
    if (t.n_faces == 0) {
        RA_HIP(hipMemsetAsync(dpos, 0, (size_t)B * V * 4 * sizeof(float), s));
        return 0;
    }
    RA_CHECK(pos && uv && face && duv, "ra_rasterize_backward: null argument (pos, uv, face, duv)");
    int err = 0;
    float* g_face = c->buf<float>("raster_g_face", (size_t)B * t.n_faces * 9, &err);
    RA_CHECK(!err, "ra_rasterize_backward: out of device memory");
    unsigned long long* sorted = nullptr;
    const int rc = raster_pixel_runs(c, face, B, t.n_faces, H, W, &sorted, s);
    RA_CHECK(rc != 1, "ra_rasterize_backward: out of device memory");
    RA_CHECK(rc == 0, "ra_rasterize_backward: device sort failed");
    RasterBwdJob j{};
    j.pos = pos; j.uv = uv; j.duv = duv; j.B = B; j.H = H; j.W = W; j.dpos = dpos;
    launch_rasterize_backward(j, t, sorted, g_face, s);
    RA_HIP(hipGetLastError());
    return 0;
}

// ---- silhouette antialiasing (ra_antialias.hip) ----------------------------------------------------
static bool antialias_sizes_ok(int C, int B, int V, int H, int W) {
    return C >= 1 && B >= 0 && V >= 0 && H >= 0 && W >= 0 && (long long)B * H < (1ll << 31) && (long long)B * H * W < (1ll << 31) &&
           (long long)B * H * W * C < (1ll << 31);
}

int ra_antialias(ra_ctx* c, const ra_topo* topo, const float* color, int C, const float* pos, int B, int V, const float* zw, const int* face, int H, int W,
                 float* out, void* stream) {
    RA_CHECK(antialias_sizes_ok(C, B, V, H, W), "ra_antialias: bad sizes (C >= 1, B, H, W >= 0, B x H x W x C < 2^31)");
    RA_CHECK(c && topo, "ra_antialias: null argument");
    RA_CHECK(owned(c->topos, topo), "ra_antialias: not a topology of this ctx");
    const TopoView& t = topo->view;
    RA_CHECK(V == t.n_verts, "ra_antialias: bad sizes (n_verts of the topology)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    const size_t n = (size_t)B * H * W * C;
    if (n == 0) return 0;
    RA_CHECK(color && out, "ra_antialias: null argument (color, out)");
    if (t.n_faces == 0) {
        RA_HIP(hipMemcpyAsync(out, color, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        return 0;
    }
    RA_CHECK(pos && zw && face, "ra_antialias: null argument (pos, zw, face)");
    AaJob j{};
    j.color = color; j.pos = pos; j.zw = zw; j.face = face; j.B = B; j.H = H; j.W = W; j.C = C;
    launch_antialias_gather(j, t, nullptr, out, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_antialias_backward(ra_ctx* c, const ra_topo* topo, const float* color, int C, const float* pos, int B, int V, const float* zw, const int* face, int H,
                          int W, const float* dout, float pos_gradient_boost, float* dcolor, float* dpos, void* stream) {
    RA_CHECK(antialias_sizes_ok(C, B, V, H, W), "ra_antialias_backward: bad sizes (C >= 1, B, H, W >= 0, B x H x W x C < 2^31)");
    RA_CHECK(c && topo, "ra_antialias_backward: null argument");
    RA_CHECK(owned(c->topos, topo), "ra_antialias_backward: not a topology of this ctx");
    const TopoView& t = topo->view;
    const long long n_pix = (long long)B * H * W;
    RA_CHECK(V == t.n_verts && (!dpos || (n_pix < (1ll << 30) && (long long)B * t.n_faces < (1ll << 29) &&
                                          (double)B * 3.0 * t.n_faces * 2.0 * H * W < 9.0e18)),
             "ra_antialias_backward: bad sizes (n_verts of the topology; with dpos B x H x W < 2^30, B x F < 2^29, 6 B F H W < 2^63)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    const size_t n = (size_t)n_pix * C;
    if (n == 0 || t.n_faces == 0) {             // no pixel or no face: no pair.  An output of no elements may be null
        if (dcolor && n > 0) {
            RA_CHECK(dout, "ra_antialias_backward: null argument (dout)");
            RA_HIP(hipMemcpyAsync(dcolor, dout, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        if (dpos && (size_t)B * V > 0) RA_HIP(hipMemsetAsync(dpos, 0, (size_t)B * V * 4 * sizeof(float), s));
        return 0;
    }
    RA_CHECK(dcolor || dpos, "ra_antialias_backward: null argument");
    RA_CHECK(color && pos && zw && face && dout, "ra_antialias_backward: null argument (color, pos, zw, face, dout)");
    AaJob j{};
    j.color = color; j.pos = pos; j.zw = zw; j.face = face; j.B = B; j.H = H; j.W = W; j.C = C;
    if (dcolor) launch_antialias_gather(j, t, dout, dcolor, s);
    if (dpos) {
        int err = 0;
        size_t tb = antialias_temp_bytes(2 * n_pix, 0);
        unsigned long long* keys = c->buf<unsigned long long>("antialias_keys", 2 * (size_t)n_pix, &err);
        unsigned long long* compact = c->buf<unsigned long long>("antialias_keys_active", 2 * (size_t)n_pix, &err);
        int* count = c->buf<int>("antialias_count", 1, &err);
        void* temp = c->buf<char>("antialias_tmp", tb + 16, &err);
        float* g_he = c->buf<float>("antialias_g_he", (size_t)B * t.n_faces * 18, &err);
        RA_CHECK(!err, "ra_antialias_backward: out of device memory");
        RA_CHECK(launch_antialias_keys(j, t, keys, compact, count, temp, tb, s) == 0, "ra_antialias_backward: device compaction failed");
        RA_HIP(hipGetLastError());
        int n_active = 0;           // the one read-back: the number of active pairs, which sizes the sort and the run pass
        RA_HIP(hipMemcpyAsync(&n_active, count, sizeof(int), hipMemcpyDeviceToHost, s));
        RA_HIP(hipStreamSynchronize(s));
        RA_CHECK(n_active >= 0 && n_active <= 2 * n_pix, "ra_antialias_backward: device compaction failed");
        tb = antialias_temp_bytes(0, n_active);
        unsigned long long* sorted = c->buf<unsigned long long>("antialias_keys_sorted", (size_t)n_active + 1, &err);
        temp = c->buf<char>("antialias_sort_tmp", tb + 16, &err);
        RA_CHECK(!err, "ra_antialias_backward: out of device memory");
        RA_CHECK(launch_antialias_dpos(j, t, dout, pos_gradient_boost, compact, sorted, n_active, temp, tb, g_he, dpos, s) == 0,
                 "ra_antialias_backward: device sort failed");
    }
    RA_HIP(hipGetLastError());
    return 0;
}

// ---- the texture path (ra_texture.hip) ------------------------------------------------------------
int ra_texture_tile(int which) { return which == 0 ? TEX_MAX_CHANNELS : which == 1 ? TEX_MAX_LEVELS : which == 2 ? TEX_MAX_EXTENT : which == 3 ? TEX_GROUP : 0; }

int ra_raster_db(ra_ctx* c, const float* pos, int B, int V, const int* faces, int F, const int* face, int H, int W, float* rast_db, void* stream) {
    RA_CHECK(raster_sizes_ok(B, H, W) && (long long)B * H * W < (1ll << 29) && V >= 0 && V < (1 << 29) && F >= 0 && F < RASTER_MAX_FACES,
             "ra_raster_db: bad sizes (B, H, W >= 1, B x H x W < 2^29, F < 2^24)");
    RA_CHECK(c && face && rast_db, "ra_raster_db: null argument");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    if (F == 0 || V == 0) {
        RA_HIP(hipMemsetAsync(rast_db, 0, (size_t)B * H * W * 4 * sizeof(float), s));
        return 0;
    }
    RA_CHECK(pos && faces, "ra_raster_db: null argument (pos, faces)");
    launch_raster_db(pos, B, V, faces, F, face, H, W, rast_db, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_interpolate_da(ra_ctx* c, const float* attr, int per_view, int V, int A, const int* faces, int F, const int* face, const float* rast_db, int B, int H,
                      int W, const int* channels, int n, float* out_da, void* stream) {
    RA_CHECK(raster_sizes_ok(B, H, W) && V >= 0 && V < (1 << 29) && F >= 0 && F < RASTER_MAX_FACES && A >= 1 && (long long)B * V * A < (1ll << 40) && n >= 1 &&
             n <= TEX_MAX_CHANNELS && (long long)B * H * W * 2 * n < (1ll << 31),
             "ra_interpolate_da: bad sizes (B, H, W >= 1, F < 2^24, A >= 1, 1 <= n <= 64, B x H x W x 2 n < 2^31)");
    RA_CHECK(channels && out_da, "ra_interpolate_da: null argument");
    for (int k = 0; k < n; ++k) RA_CHECK(channels[k] >= 0 && channels[k] < A, "ra_interpolate_da: bad sizes (a selected channel outside [0, A))");
    RA_CHECK(c, "ra_interpolate_da: null argument");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    if (F == 0 || V == 0) {
        RA_HIP(hipMemsetAsync(out_da, 0, (size_t)B * H * W * 2 * n * sizeof(float), s));
        return 0;
    }
    RA_CHECK(attr && faces && face && rast_db, "ra_interpolate_da: null argument (attr, faces, face, rast_db)");
    TexDaJob j{};
    j.attr = attr; j.faces = faces; j.face = face; j.rast_db = rast_db; j.per_view = per_view != 0; j.V = V; j.A = A; j.F = F; j.B = B; j.H = H; j.W = W; j.n = n;
    for (int k = 0; k < n; ++k) j.ch[k] = channels[k];
    launch_interpolate_da(j, out_da, s);
    RA_HIP(hipGetLastError());
    return 0;
}

static bool texture_tex_ok(int Bt, int TH, int TW, int C, int max_mip_level) {
    return Bt >= 1 && TH >= 1 && TW >= 1 && TH <= TEX_MAX_EXTENT && TW <= TEX_MAX_EXTENT && C >= 1 && C <= TEX_MAX_CHANNELS && max_mip_level >= 0 &&
           (long long)Bt * TH * TW * C < (1ll << 31);
}

int ra_texture_mips(ra_ctx* c, const float* tex, int Bt, int TH, int TW, int C, int max_mip_level, float* mips, int* lmax, long long* offsets, void* stream) {
    RA_CHECK(texture_tex_ok(Bt, TH, TW, C, max_mip_level),
             "ra_texture_mips: bad sizes (Bt >= 1, 1 <= TH, TW <= 32768, 1 <= C <= 64, max_mip_level >= 0, Bt x TH x TW x C < 2^31)");
    RA_CHECK(lmax && offsets, "ra_texture_mips: null argument");
    TexLevels L;
    texture_levels(TH, TW, max_mip_level, L);
    *lmax = L.n - 1;
    for (int l = 0; l <= L.n; ++l) offsets[l] = L.off[l];
    if (!mips) return 0;                // the sizes alone
    RA_CHECK(c && tex, "ra_texture_mips: null argument (ctx, tex)");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    const long long total = L.off[L.n] * C, level0 = L.off[1] * C;
    for (int bt = 0; bt < Bt; ++bt)
        RA_HIP(hipMemcpyAsync(mips + (long long)bt * total, tex + (long long)bt * level0, (size_t)level0 * sizeof(float), hipMemcpyDeviceToDevice, s));
    for (int l = 1; l < L.n; ++l) launch_texture_mip(mips + L.off[l - 1] * C, total, mips + L.off[l] * C, total, Bt, L.h[l], L.w[l], C, s);
    RA_HIP(hipGetLastError());
    return 0;
}

// the job of ra_texture and ra_texture_backward: the chain of a trilinear call goes to the ctx's scratch
static int texture_job(ra_ctx* c, const char* who, const float* tex, int Bt, int TH, int TW, int C, const float* uv, const float* uv_da, int B, int H, int W,
                       int filter, int boundary, int max_mip_level, TexJob* j, hipStream_t s) {
    j->tex = tex; j->uv = uv; j->uv_da = uv_da; j->Bt = Bt; j->B = B; j->H = H; j->W = W; j->C = C; j->filter = filter; j->boundary = boundary;
    texture_levels(TH, TW, filter == TEX_TRILINEAR ? max_mip_level : 0, j->L);
    if (j->L.n > 1) {
        int err = 0;
        const long long stride = (j->L.off[j->L.n] - j->L.off[1]) * C;
        float* mips = c->buf<float>("texture_mips", (size_t)Bt * stride, &err);
        if (err) { ra_set_error(std::string(who) + ": out of device memory"); return 1; }
        launch_texture_mip(tex, j->L.off[1] * C, mips, stride, Bt, j->L.h[1], j->L.w[1], C, s);
        for (int l = 2; l < j->L.n; ++l)
            launch_texture_mip(mips + (j->L.off[l - 1] - j->L.off[1]) * C, stride, mips + (j->L.off[l] - j->L.off[1]) * C, stride, Bt, j->L.h[l], j->L.w[l], C, s);
        j->mips = mips;
    }
    return 0;
}

static bool texture_sizes_ok(int Bt, int TH, int TW, int C, int B, int H, int W, int max_mip_level) {
    return texture_tex_ok(Bt, TH, TW, C, max_mip_level) && raster_sizes_ok(B, H, W) && (Bt == 1 || Bt == B) && (long long)B * H * W * C < (1ll << 31);
}
#define RA_TEXTURE_SIZES "bad sizes (Bt = 1 or B, 1 <= TH, TW <= 32768, 1 <= C <= 64, max_mip_level >= 0, Bt x TH x TW x C < 2^31, B, H, W >= 1, B x H x W x C < 2^31"

int ra_texture(ra_ctx* c, const float* tex, int Bt, int TH, int TW, int C, const float* uv, const float* uv_da, int B, int H, int W, int filter, int boundary,
               int max_mip_level, float* out, void* stream) {
    RA_CHECK(texture_sizes_ok(Bt, TH, TW, C, B, H, W, max_mip_level), "ra_texture: " RA_TEXTURE_SIZES ")");
    RA_CHECK(filter >= TEX_NEAREST && filter <= TEX_TRILINEAR && boundary >= TEX_WRAP && boundary <= TEX_CLAMP, "ra_texture: unknown mode");
    RA_CHECK(c && tex && uv && out && (uv_da || filter != TEX_TRILINEAR), "ra_texture: null argument");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    TexJob j{};
    if (texture_job(c, "ra_texture", tex, Bt, TH, TW, C, uv, uv_da, B, H, W, filter, boundary, max_mip_level, &j, s)) return 1;
    launch_texture(j, out, s);
    RA_HIP(hipGetLastError());
    return 0;
}

int ra_texture_backward(ra_ctx* c, const float* tex, int Bt, int TH, int TW, int C, const float* uv, const float* uv_da, int B, int H, int W, int filter,
                        int boundary, int max_mip_level, const float* dout, float* duv, float* dtex, void* stream) {
    // the tap-count limit: the B H W T tap slots (T = 1, 4, 8 by filter) are sorted as ONE array of 64-bit keys indexed by an int
    const long long taps = (long long)B * H * W * texture_taps_per_pixel(filter);
    TexLevels L;
    if (TH >= 1 && TW >= 1 && max_mip_level >= 0) texture_levels(TH, TW, filter == TEX_TRILINEAR ? max_mip_level : 0, L); else { L.n = 1; L.off[1] = 1; }
    RA_CHECK(texture_sizes_ok(Bt, TH, TW, C, B, H, W, max_mip_level) &&
             (!dtex || (taps < (1ll << 31) - 1 && (double)B * (double)L.off[L.n] * (double)taps < 9.0e18 && (long long)B * L.off[L.n] * C < (1ll << 40))),
             "ra_texture_backward: " RA_TEXTURE_SIZES "; with dtex B x H x W x taps < 2^31 - 1 (taps 1, 4, 8 by filter) and B x texels x B x H x W x taps < 2^63)");
    RA_CHECK(filter >= TEX_NEAREST && filter <= TEX_TRILINEAR && boundary >= TEX_WRAP && boundary <= TEX_CLAMP, "ra_texture_backward: unknown mode");
    RA_CHECK(c && tex && uv && dout && (duv || dtex) && (uv_da || filter != TEX_TRILINEAR), "ra_texture_backward: null argument");
    hipStream_t s = (hipStream_t)stream;
    RA_HIP(hipSetDevice(c->device));
    TexJob j{};
    if (texture_job(c, "ra_texture_backward", tex, Bt, TH, TW, C, uv, uv_da, B, H, W, filter, boundary, max_mip_level, &j, s)) return 1;
    if (duv) launch_texture_duv(j, dout, duv, s);
    if (dtex) {
        int err = 0;
        const size_t tb = texture_temp_bytes(taps);
        unsigned long long* keys = c->buf<unsigned long long>("texture_keys", (size_t)taps, &err);
        unsigned long long* sorted = c->buf<unsigned long long>("texture_keys_sorted", (size_t)taps, &err);
        void* temp = c->buf<char>("texture_sort_tmp", tb + 16, &err);
        float* g = c->buf<float>("texture_g", (size_t)B * j.L.off[j.L.n] * C, &err);
        RA_CHECK(!err, "ra_texture_backward: out of device memory");
        RA_CHECK(launch_texture_dtex(j, dout, keys, sorted, temp, tb, g, dtex, s) == 0, "ra_texture_backward: device sort failed");
    }
    RA_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
