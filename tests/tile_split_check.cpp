// CPU check of the dense GEMM's tile lists (csrc/model_tables.h: tile_key / tile_rest) on tiny descriptors: the two lists
// partition the ceil(V / 16) tiles, both ascend, a tile is a key tile exactly when it holds an exported vertex (vslot >= 0).
// Cases: V no multiple of 16 with static and dynamic landmarks, an empty key list (every keypoint a kinematic joint), every
// tile a key tile, V a multiple of 16.  Stand-alone: own main, no device.  Built and run by tests/test_tile_split_host.py
// (product and -DSFX_LAB form, host AddressSanitizer + UBSan).
#include "../smplify-x-partial_amd/csrc/model_tables.h"
#include <cstdarg>
#include <cstdio>
#include <set>

static char g_msg[512];
void sfx_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_msg, sizeof(g_msg), fmt, ap); va_end(ap); }

static int g_fail = 0, g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { if (++g_fail <= 40) printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); } } while (0)

enum { S = 4, P = 9 * (SFX_J - 1), ROWS = 2 };

struct Desc {       // owns the arrays a sfx_model_desc points to
    int V = 0, F = 0;
    std::vector<float> vt, sd, pd, jr, W, cl, cr, pm, lb, db;
    std::vector<int> par, faces, extra, lf, df, jm;
    sfx_model_desc d{};
    const sfx_model_desc* get() {
        d.V = V; d.F = F; d.J = SFX_J; d.num_betas = 2; d.num_expr = S - 2; d.num_pca = 2;
        d.v_template = vt.data(); d.shapedirs = sd.data(); d.posedirs = pd.data(); d.J_regressor = jr.data();
        d.lbs_weights = W.data(); d.parents = par.data(); d.hands_comp_l = cl.data(); d.hands_comp_r = cr.data();
        d.pose_mean = pm.data(); d.faces = faces.data(); d.n_extra = (int)extra.size(); d.extra_vertex_ids = extra.data();
        d.n_lmk = (int)lf.size(); d.lmk_faces_idx = lf.data(); d.lmk_bary = lb.data();
        d.n_dyn = (int)(df.size() / ROWS); d.n_dyn_rows = ROWS; d.dyn_lmk_faces_idx = df.data(); d.dyn_lmk_bary = db.data();
        d.K = (int)jm.size(); d.joint_map = jm.data();
        return &d;
    }
};

// V vertices, one skinning weight each; face f = (3f, 3f + 1, 3f + 2) mod V; keypoints: two kinematic joints, then the extra
// vertices, the static landmarks (faces lf) and the dynamic ones (faces df, [ROWS][n_dyn])
static Desc make_desc(int V, std::vector<int> extra, std::vector<int> lf, std::vector<int> df) {
    Desc D; D.V = V; D.F = (V + 2) / 3;
    unsigned seed = 977u + (unsigned)V;
    auto fill = [&](std::vector<float>& a, size_t n) { a.resize(n); for (float& x : a) { seed = seed * 1664525u + 1013904223u; x = (float)((seed >> 8) & 0xffff) / 65536.f - 0.5f; } };
    fill(D.vt, (size_t)V * 3); fill(D.sd, (size_t)V * 3 * S); fill(D.pd, (size_t)V * 3 * P); fill(D.cl, 2 * SFX_NHAND); fill(D.cr, 2 * SFX_NHAND);
    fill(D.pm, SFX_POSE); fill(D.jr, (size_t)SFX_J * V);
    D.W.assign((size_t)V * SFX_J, 0.f);
    for (int v = 0; v < V; ++v) D.W[(size_t)v * SFX_J + v % SFX_J] = 1.f;
    D.par.resize(SFX_J); for (int j = 0; j < SFX_J; ++j) D.par[j] = j ? (j - 1) / 2 : -1;
    for (int f = 0; f < D.F; ++f) for (int c = 0; c < 3; ++c) D.faces.push_back((3 * f + c) % V);
    D.extra = extra; D.lf = lf; D.df = df;
    fill(D.lb, lf.size() * 3); fill(D.db, df.size() * 3);
    D.jm = {0, 7};
    const int e0 = SFX_J, l0 = e0 + (int)extra.size(), d0 = l0 + (int)lf.size(), end = d0 + (int)(df.size() / ROWS);
    for (int s = e0; s < end; ++s) D.jm.push_back(s);
    return D;
}

// expect_key: the key list the case was built to give
static void check(const char* name, Desc D, const std::vector<int>& expect_key) {
    ModelTables T;
    const int rc = sfx_build_model_tables(D.get(), &T);
    CHECK(rc == 0);
    if (rc) { printf("%s: refused: %s\n", name, g_msg); return; }
    const int V = D.V, nt = (V + 15) / 16;
    CHECK((int)T.vslot.size() == T.Vpad && T.Vpad >= nt * 16);
    CHECK((int)(T.tile_key.size() + T.tile_rest.size()) == nt);
    std::vector<int> seen(nt, 0);
    for (const std::vector<int>* l : {&T.tile_key, &T.tile_rest})
        for (size_t i = 0; i < l->size(); ++i) {
            const int t = (*l)[i];
            CHECK(t >= 0 && t < nt);
            if (t >= 0 && t < nt) ++seen[t];
            if (i) CHECK(t > (*l)[i - 1]);                     // ascending (hence no tile twice within a list)
        }
    for (int t = 0; t < nt; ++t) CHECK(seen[t] == 1);           // key and rest together cover every tile exactly once
    const std::set<int> key(T.tile_key.begin(), T.tile_key.end());
    int exported = 0;
    for (int v = 0; v < T.Vpad; ++v) {
        if (v >= V) { CHECK(T.vslot[v] == -1); continue; }
        if (T.vslot[v] >= 0) { ++exported; CHECK(key.count(v / 16) == 1); }      // every exported vertex lies in a key tile
    }
    CHECK(exported == T.n_uniq);
    for (int t : T.tile_key) {                                  // no key tile without an exported vertex
        bool any = false;
        for (int q = 0; q < 16; ++q) any = any || (t * 16 + q < V && T.vslot[t * 16 + q] >= 0);
        CHECK(any);
    }
    CHECK(T.tile_key == expect_key);
    printf("%s: V %d, %d tiles, %zu key, %zu rest, %d exported vertices\n", name, V, nt, T.tile_key.size(), T.tile_rest.size(), T.n_uniq);
}

int main() {
    // V = 100: seven tiles, the last with four vertices.  Extra vertices 5 and 99 (tiles 0 and 6), the static landmark on face 11
    // (vertices 33 .. 35: tile 2), a dynamic landmark on face 16 in one LUT row (48 .. 50: tile 3) and on face 26 in the other
    // (78 .. 80: tiles 4 and 5) -- tile 1 alone has no consumer
    check("ragged", make_desc(100, {5, 99}, {11}, {16, 26}), {0, 2, 3, 4, 5, 6});
    // every keypoint a kinematic joint: nothing is exported, the key list is empty (the loop then skips the key launch)
    check("no-items", make_desc(100, {}, {}, {}), {});
    // every tile a key tile: the rest list is empty; V = 40 leaves eight vertices in the last tile
    check("all-key", make_desc(40, {0, 16, 39}, {}, {}), {0, 1, 2});
    // V a multiple of 16 (and of 32: Vpad == V), one exported vertex in the last tile, as its last vertex
    check("full-tiles", make_desc(64, {63}, {}, {}), {3});
    // V = 17: the second tile holds one vertex, and it is the exported one
    check("one-over", make_desc(17, {16}, {}, {}), {1});
    printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
