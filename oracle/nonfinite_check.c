/*
 * nonfinite_check.c -- stand-alone driver of the CPU oracle on coordinates that are not finite (test infrastructure only).
 * Built with -fsanitize=undefined,float-cast-overflow -fno-sanitize-recover=all together with tsl_oracle.c and tsl_oracle_octo.c
 * (`make -C oracle nonfinite-check`; tests/test_limit_scenes_cpu.py does so where the compiler has the sanitizer): the oracle must
 * turn such a coordinate into "outside" without ever casting it.  Prints the counts it checks; exit code 0 = as expected.
 */
#include "tsl_oracle.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define NBAD 13
static const float BAD[NBAD][3] = {
    { NAN, 0.5f, 0.5f }, { 0.5f, NAN, 0.5f }, { 0.5f, 0.5f, NAN }, { NAN, NAN, NAN }, { INFINITY, 0.0f, 0.0f }, { 0.0f, -INFINITY, 0.0f },
    { 0.5f, 0.5f, INFINITY }, { -INFINITY, INFINITY, 0.0f }, { 1e12f, 0.0f, 0.0f }, { 0.0f, -1e12f, 0.5f }, { 0.5f, 0.0f, 1e12f },
    { 3e38f, 1.0f, 1.0f }, { 1.0f, 1.0f, -3e38f } };

static unsigned lcg(unsigned* s) { *s = *s * 1664525u + 1013904223u; return *s >> 8; }
static float uni(unsigned* s, float lo, float hi) { return lo + (hi - lo) * (float)(lcg(s) & 0xffffu) / 65536.0f; }

enum { NV = 2000, NOWN = NV + NBAD + 2 };

/* everything the oracle does with caller coordinates, on the cloud xyz[n][3]; check = the cloud is the built-in one (NV valid points, BAD, -0.0, 10 m out): verify the counts */
static int run(const float (*xyz)[3], int N, int check)
{
    const double I3[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, Z3[3] = { 0, 0, 0 };
    int fail = 0;

    /* the Octomap: a cloud, and a fusion under a base pose that carries the leaves beyond any int */
    ora_octo_cfg oc; memset(&oc, 0, sizeof(oc));
    oc.map_size_xy = 12.8; oc.map_size_z = 12.8; oc.voxel_scale = 0.05; oc.min_ray_length = 0.3; oc.max_ray_length = 5.0; oc.K = 2; oc.max_submap_num = 2; oc.recast_step = 2;
    ora_octo* o = ora_octo_create(&oc);
    ora_frame_stats st;
    ora_octo_integrate_points(o, I3, Z3, &xyz[0][0], NULL, N, &st);
    printf("octomap: p_used %lld p_valid %lld p_oob %lld\n", (long long)st.p_used, (long long)st.p_valid, (long long)st.p_oob);
    if (check) fail |= st.p_oob != NBAD + 1 || st.p_valid != NV + 1;
    ora_octo_set_active_submap(o, 1);
    oc.is_global_map = 1;
    ora_octo* g = ora_octo_create(&oc);
    const double far[3] = { 1e12, 0, 0 }, nanT[3] = { NAN, 0, 0 };
    ora_octo_set_base_pose_submap(g, 0, I3, far);
    ora_octo_fuse_submaps(g, o);
    fail |= ora_octo_export_leaves(g, NULL, NULL, NULL, 0) != 0;
    ora_octo_set_base_pose_submap(g, 0, I3, nanT);
    ora_octo_fuse_submaps(g, o);
    fail |= ora_octo_export_leaves(g, NULL, NULL, NULL, 0) != 0;
    ora_octo_destroy(g); ora_octo_destroy(o);

    /* the TSDF: the cloud is gated; the queries read "outside"; rays from and towards such coordinates */
    ora_tsdf_cfg tc; memset(&tc, 0, sizeof(tc));
    tc.map_size_xy = 10.24; tc.map_size_z = 10.24; tc.voxel_scale = 0.04; tc.num_voxel_per_blk_axis = 16; tc.max_ray_length = 5.0; tc.min_ray_length = 0.3;
    tc.internal_voxels = 10; tc.max_submap_num = 2; tc.recast_step = 2; tc.disp_ceiling = 1.8; tc.disp_floor = -0.3;
    ora_tsdf* m = ora_tsdf_create(&tc);
    ora_tsdf_integrate_points(m, ORA_BATCHED, I3, Z3, &xyz[0][0], NULL, N, &st);
    printf("tsdf: p_used %lld p_valid %lld p_oob %lld\n", (long long)st.p_used, (long long)st.p_valid, (long long)st.p_oob);
    fail |= st.p_used != N || (check && st.p_valid + st.p_oob > NV + 1);
    uint8_t* out = (uint8_t*)calloc((size_t)N, 1);
    for (int mode = 0; mode < 3; ++mode) {
        ora_tsdf_query_points(m, mode, mode == 2 ? 2 : 0, &xyz[0][0], N, out);
        int ones = 0; for (int q = NV; check && q < NV + NBAD; ++q) ones += out[q];
        printf("query mode %d: %d of %d bad points read as outside\n", mode, ones, NBAD);
        if (check) fail |= ones != NBAD;
    }
    { uint8_t b16[NBAD]; ora_tsdf_query_points(m, 2, 16, &BAD[0][0], NBAD, b16); for (int q = 0; q < NBAD; ++q) fail |= b16[q] != 1; }      /* the widest neighbourhood, on the bad points alone */
    float (*dir)[3] = calloc((size_t)N, sizeof(*dir)); float (*end)[3] = calloc((size_t)N, sizeof(*end)); float* len = calloc((size_t)N, sizeof(float)); uint8_t* hit = calloc((size_t)N, 1);
    for (int q = 0; q < N; ++q) for (int a = 0; a < 3; ++a) dir[q][a] = xyz[(q * 7 + 3) % N][(a + 1) % 3];
    const float dists[] = { 0.0f, 0.03f, 4.0f, -1.0f, NAN, INFINITY };
    for (unsigned k = 0; k < sizeof(dists) / sizeof(dists[0]); ++k) ora_tsdf_query_raycast(m, &xyz[0][0], &dir[0][0], dists[k], N, hit, &end[0][0], len);
    ora_tsdf_query_raycast(m, &xyz[0][0], &dir[0][0], 4.0f, N, hit, &end[0][0], len);
    int hits = 0; for (int q = NV; check && q < NV + NBAD; ++q) hits += hit[q];
    printf("raycast: %d of %d rays from bad origins hit at once\n", hits, NBAD);
    if (check) fail |= hits != NBAD;
    ora_tsdf_destroy(m);
    free(out); free(dir); free(end); free(len); free(hit);
    return fail;
}

/* no argument: the built-in cloud, counts verified.  Arguments: files of raw float32 triples (the clouds of the GPU tests), run for the sanitizer's sake. */
int main(int argc, char** argv)
{
    static float own[NOWN][3];
    unsigned seed = 7u;
    for (int q = 0; q < NV; ++q) for (int a = 0; a < 3; ++a) own[q][a] = uni(&seed, -2.5f, 2.5f);
    memcpy(own[NV], BAD, sizeof(BAD));
    own[NV + NBAD][0] = -0.0f; own[NV + NBAD][1] = -0.0f; own[NV + NBAD][2] = -0.0f;
    own[NV + NBAD + 1][0] = 10.0f; own[NV + NBAD + 1][1] = -10.0f; own[NV + NBAD + 1][2] = 10.0f;
    int fail = run((const float (*)[3])own, NOWN, 1);
    for (int k = 1; k < argc; ++k) {
        FILE* f = fopen(argv[k], "rb");
        if (!f) { printf("cannot open %s\n", argv[k]); return 2; }
        fseek(f, 0, SEEK_END); long bytes = ftell(f); fseek(f, 0, SEEK_SET);
        int n = (int)(bytes / 12);
        float (*xyz)[3] = malloc((size_t)(n > 0 ? n : 1) * 12);
        if (fread(xyz, 12, (size_t)n, f) != (size_t)n) { printf("short read of %s\n", argv[k]); return 2; }
        fclose(f);
        printf("%s: %d points\n", argv[k], n);
        fail |= run((const float (*)[3])xyz, n, 0);
        free(xyz);
    }
    printf(fail ? "FAILED\n" : "ok\n");
    return fail;
}
