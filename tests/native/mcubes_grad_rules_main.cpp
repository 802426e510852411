// A stand-alone CPU program around csrc/ra_mcubes_grad_rules.hpp (built with -fsanitize=address,undefined by
// tests/test_oracle_mcubes_grad.py).  It reads one case from the file named on its command line — whitespace-separated tokens, every
// float as the hexadecimal bits of its fp32 value:
//     nx ny nz C V has_dverts iso, volume (nx ny nz), dverts (V 3, when has_dverts), attrs (nx ny nz C), dattr (V C)
// classifies and sums the volume as the kernels do, runs the gather of ra_mcubes_grad.hip one grid point at a time, and prints, for the
// test to compare bit for bit with the float32 restatement (tests/mcubes_grad_ref.py):
//     verts <n>                   the crossed edges it counted (must be V)
//     dvol <bits> ...             n values
//     dA <bits> ...               n C values
//     attr <bits> ...             V C values
#include "ra_mcubes_grad_rules.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

static unsigned bits(float x) { unsigned u; std::memcpy(&u, &x, 4); return u; }
static bool read_float(std::FILE* f, float* x) {
    unsigned u;
    if (std::fscanf(f, "%x", &u) != 1) return false;
    std::memcpy(x, &u, 4);
    return true;
}
static bool read_floats(std::FILE* f, std::vector<float>& v) {
    for (float& x : v) if (!read_float(f, &x)) return false;
    return true;
}
static void print(const char* name, const std::vector<float>& v) {
    std::printf("%s", name);
    for (float x : v) std::printf(" %08x", bits(x));
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 2) { std::printf("usage: mcubes_grad_rules_main <case file>\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    int nx, ny, nz, C, V, has_dverts;
    float iso;
    if (std::fscanf(f, "%d %d %d %d %d %d", &nx, &ny, &nz, &C, &V, &has_dverts) != 6 || !read_float(f, &iso) || nx < 2 || ny < 2 || nz < 2 || C < 0 ||
        C > MCG_MAX_C || V < 0) {
        std::printf("bad header\n");
        return 2;
    }
    const int n = nx * ny * nz;
    std::vector<float> vol(n), dverts(has_dverts ? (size_t)3 * V : 0), A((size_t)n * C), dattr((size_t)V * C);
    if (!read_floats(f, vol) || !read_floats(f, dverts) || !read_floats(f, A) || !read_floats(f, dattr)) { std::printf("short case file\n"); return 2; }
    std::fclose(f);

    const int stride[3] = {ny * nz, nz, 1}, dim[3] = {nx, ny, nz};
    std::vector<unsigned> mask(n), off(n + 1);
    unsigned total = 0;
    for (int p = 0; p < n; ++p) {
        const int coord[3] = {p / (nz * ny), (p / nz) % ny, p % nz};
        unsigned m = 0;
        for (int k = 0; k < 3; ++k)
            if (coord[k] + 1 < dim[k] && mcg_crossed(vol[p], vol[p + stride[k]], iso)) m |= 1u << k;
        mask[p] = m; off[p] = total; total += mcg_popc3(m);
    }
    off[n] = total;
    std::printf("verts %u\n", total);

    std::vector<float> dvol(n), dA((size_t)n * C), attr((size_t)V * C);
    for (int p = 0; p < n; ++p) {
        const int coord[3] = {p / (nz * ny), (p / nz) % ny, p % nz};
        McgEdge e[6];
        bool on[6];
        unsigned v[6];
        int other[6];
        for (int k = 0; k < 3; ++k) {
            on[k] = false; v[k] = 0; other[k] = p;
            if ((mask[p] >> k) & 1u) {
                v[k] = off[p] + mcg_slot(mask[p], k);
                other[k] = p + stride[k];
                if (v[k] < (unsigned)V) {
                    on[k] = mcg_edge(vol[p], vol[other[k]], iso, e[k]);
                    for (int c = 0; c < C; ++c) attr[(size_t)v[k] * C + c] = mcg_attr(e[k], A[(size_t)p * C + c], A[(size_t)other[k] * C + c]);
                }
            }
        }
        for (int k = 0; k < 3; ++k) {
            on[3 + k] = false; v[3 + k] = 0; other[3 + k] = p;
            if (coord[k] > 0) {
                const int pm = p - stride[k];
                if ((mask[pm] >> k) & 1u) {
                    v[3 + k] = off[pm] + mcg_slot(mask[pm], k);
                    other[3 + k] = pm;
                    if (v[3 + k] < (unsigned)V) on[3 + k] = mcg_edge(vol[pm], vol[p], iso, e[3 + k]);
                }
            }
        }
        float gt[6];
        for (int i = 0; i < 6; ++i) gt[i] = (on[i] && has_dverts) ? dverts[3 * (size_t)v[i] + i % 3] : 0.0f;
        for (int c = 0; c < C; ++c) {
            const float mine = A[(size_t)p * C + c];
            float acc = 0.0f;
            for (int i = 0; i < 6; ++i) {
                if (!on[i]) continue;
                const float theirs = A[(size_t)other[i] * C + c], g = dattr[(size_t)v[i] * C + c];
                if (i < 3) { gt[i] = mcg_gt_add(gt[i], g, mine, theirs); acc = acc + mcg_dAp(e[i], g); }
                else       { gt[i] = mcg_gt_add(gt[i], g, theirs, mine); acc = acc + mcg_dAq(e[i], g); }
            }
            dA[(size_t)p * C + c] = acc;
        }
        float acc = 0.0f;
        for (int i = 0; i < 6; ++i) {
            if (!on[i]) continue;
            const float s = mcg_s(e[i], gt[i]);
            acc = acc + (i < 3 ? mcg_ca(e[i], s) : mcg_cb(e[i], s));
        }
        dvol[p] = acc;
    }
    print("dvol", dvol);
    print("dA", dA);
    print("attr", attr);
    return 0;
}
