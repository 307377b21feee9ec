// Stand-alone host run of the custom vial's mesh code (drtvam_amd/csrc/tvam_mesh.hip: validation,
// the hierarchy's builder; tvam_mesh.h: its traversal and the loop over all triangles), for a
// sanitizer build without a GPU or an interpreter:
//   hipcc --cuda-host-only -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Iinclude tools/mesh_check.hip -o mesh_check && ./mesh_check
// Meshes: tessellated open tubes of 1 to 4096 triangles (every leaf size and odd counts), random
// rays with axis-parallel ones among them; the hierarchy and the loop must return the same bits.
// Prints one line per mesh; exit status 1 on a mismatch.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../drtvam_amd/csrc/tvam_mesh.hip"

static std::string g_msg;
int tvam_fail(int code, const std::string& msg) {
    g_msg = msg;
    return code;
}
int tvam_hip_fail(hipError_t, const char* what) { return tvam_fail(TVAM_ERR_HIP, what); }

static uint32_t g_state = 12345u;
static float uni() {  // xorshift32 in [0, 1)
    g_state ^= g_state << 13, g_state ^= g_state >> 17, g_state ^= g_state << 5;
    return (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

int main() {
    int bad = 0;
    for (int n_tris : {1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 33, 100, 1023, 4096}) {
        std::vector<float> tris;
        const int n_phi = 8 + n_tris / 64;
        for (int i = 0; (int)tris.size() < 9 * n_tris; ++i) {
            const int q = i / 2, a = q % n_phi, z = q / n_phi;
            const float p0 = 6.2831853f * (float)a / (float)n_phi, p1 = 6.2831853f * (float)(a + 1) / (float)n_phi;
            const float z0 = -3.0f + 0.25f * (float)z, z1 = z0 + 0.25f;
            const float A[3] = {3.0f * cosf(p0), 3.0f * sinf(p0), z0}, B[3] = {3.0f * cosf(p1), 3.0f * sinf(p1), z0};
            const float C[3] = {3.0f * cosf(p1), 3.0f * sinf(p1), z1}, D[3] = {3.0f * cosf(p0), 3.0f * sinf(p0), z1};
            const float* v[3] = {A, (i & 1) ? C : B, (i & 1) ? D : C};
            for (int k = 0; k < 3; ++k) tris.insert(tris.end(), v[k], v[k] + 3);
        }
        const int64_t n_rays = 4000;
        std::vector<float> o(3 * n_rays), d(3 * n_rays), t0(n_rays), t1(n_rays);
        std::vector<int32_t> i0(n_rays), i1(n_rays);
        for (int64_t r = 0; r < n_rays; ++r) {
            float len = 0.0f;
            for (int a = 0; a < 3; ++a) {
                o[3 * r + a] = 12.0f * uni() - 6.0f;
                d[3 * r + a] = (r % 5 == 0) ? 0.0f : 8.0f * uni() - 4.0f - o[3 * r + a];
            }
            if (r % 5 == 0) d[3 * r + (r / 5) % 3] = (r & 8) ? 1.0f : -1.0f;
            for (int a = 0; a < 3; ++a) len += d[3 * r + a] * d[3 * r + a];
            for (int a = 0; a < 3; ++a) d[3 * r + a] /= sqrtf(len);
        }
        if (tvam_mesh_hit(tris.data(), n_tris, o.data(), d.data(), n_rays, 1, t1.data(), i1.data()) ||
            tvam_mesh_hit(tris.data(), n_tris, o.data(), d.data(), n_rays, 0, t0.data(), i0.data())) {
            printf("%d triangles: refused: %s\n", n_tris, g_msg.c_str());
            bad = 1;
            continue;
        }
        int64_t hits = 0, diff = 0;
        for (int64_t r = 0; r < n_rays; ++r) {
            hits += i0[r] >= 0;
            diff += std::memcmp(&t0[r], &t1[r], sizeof(float)) != 0 || i0[r] != i1[r];
        }
        printf("%d triangles: %lld of %lld rays hit, %lld differ\n", n_tris, (long long)hits, (long long)n_rays,
               (long long)diff);
        bad |= diff != 0;
    }
    // refusals: empty, non-finite, zero area
    float tri[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0};
    bad |= tvam_mesh_validate("outer", tri, 0) != TVAM_ERR_INVALID;
    tri[4] = NAN;
    bad |= tvam_mesh_validate("outer", tri, 1) != TVAM_ERR_INVALID;
    tri[4] = 0.0f, tri[7] = 0.0f;
    bad |= tvam_mesh_validate("outer", tri, 1) != TVAM_ERR_INVALID;
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad;
}
