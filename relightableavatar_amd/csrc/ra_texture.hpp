// The texture path (ra_texture.hip): the launchers behind ra_raster_db, ra_interpolate_da, ra_texture_mips, ra_texture, ra_texture_backward
#pragma once
#include "ra_kernels.hpp"
#include "ra_texture_rules.hpp"

constexpr int TEX_BLOCK = 256;          // pixels / texels per workgroup; the run pass uses one wave
constexpr int TEX_GROUP = 4;            // channels a wave of the run pass sums per trip over its run
constexpr long long TEX_MAX_WAVES = 1ll << 24;
struct TexJob {
    const float* tex;                   // Bt x TH x TW x C: level 0
    const float* mips;                  // levels 1 .. Lmax of every texture, Bt x (L.off[L.n] - L.off[1]) x C; not read when L.n == 1
    const float* uv;                    // B x H x W x 2
    const float* uv_da;                 // B x H x W x 4; read only with TEX_TRILINEAR
    int Bt, B, H, W, C, filter, boundary;
    TexLevels L;                        // one level unless TEX_TRILINEAR
};
struct TexDaJob {
    const float* attr;                  // V x A or B x V x A
    const int* faces;                   // F x 3
    const int* face;                    // B x H x W
    const float* rast_db;               // B x H x W x 4
    int per_view, V, A, F, B, H, W, n;
    int ch[TEX_MAX_CHANNELS];
};
inline int texture_taps_per_pixel(int filter) { return filter == TEX_NEAREST ? 1 : filter == TEX_LINEAR ? 4 : 8; }
size_t texture_temp_bytes(long long n_sort);
void launch_raster_db(const float* pos, int B, int V, const int* faces, int F, const int* face, int H, int W, float* rast_db, hipStream_t s);
void launch_interpolate_da(const TexDaJob& j, float* out, hipStream_t s);
// level l + 1 of every texture from level l: src, dst point at the levels of texture 0, the strides are floats per texture; (w, h): dst's
void launch_texture_mip(const float* src, long long src_stride, float* dst, long long dst_stride, int Bt, int h, int w, int C, hipStream_t s);
void launch_texture(const TexJob& j, float* out, hipStream_t s);
void launch_texture_duv(const TexJob& j, const float* dout, float* duv, hipStream_t s);
// keys, sorted: B H W T entries; g: B x L.off[L.n] x C, zeroed here; dtex: Bt x TH x TW x C
int launch_texture_dtex(const TexJob& j, const float* dout, unsigned long long* keys, unsigned long long* sorted, void* temp, size_t temp_bytes, float* g,
                        float* dtex, hipStream_t s);
