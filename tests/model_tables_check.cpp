// CPU check of the model's host tables (csrc/model_tables.h): a tiny deterministic descriptor, every table against its
// definition recomputed the slow obvious way, the row-overflow fallback, and every refusal.  Stand-alone: own main, no device.
// Built and run by tests/test_model_tables_host.py (product and -DSFX_LAB form, host AddressSanitizer + UBSan).
#include "../smplify-x-partial_amd/csrc/model_tables.h"
#include <cstdarg>
#include <cstdio>
#include <set>
#include <string>

static char g_msg[512];
void sfx_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_msg, sizeof(g_msg), fmt, ap); va_end(ap); }

static int g_fail = 0, g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { if (++g_fail <= 40) printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); } } while (0)

enum { V = 37, F = 60, S = 4, P = 9 * (SFX_J - 1), NEXTRA = 3, NLMK = 4, ROWS = 3, NDYN = 2 };

struct Desc {       // owns the arrays a sfx_model_desc points to
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

static unsigned g_seed;
static float rnd() { g_seed = g_seed * 1664525u + 1013904223u; return (float)((g_seed >> 8) & 0xffff) / 65536.f + 0.015625f; }   // > 0
static void fill(std::vector<float>& a, size_t n) { a.resize(n); for (float& x : a) x = rnd() - 0.5f; }
static void set_weights(Desc& D, int v, int n) {     // n nonzero weights on vertex v, on distinct joints spread over the range
    for (int j = 0; j < SFX_J; ++j) D.W[(size_t)v * SFX_J + j] = 0.f;
    for (int i = 0; i < n; ++i) D.W[(size_t)v * SFX_J + (v * 7 + i * 13) % SFX_J] = rnd();
}

static Desc make_desc() {
    Desc D; g_seed = 12345u;
    fill(D.vt, V * 3); fill(D.sd, (size_t)V * 3 * S); fill(D.pd, (size_t)V * 3 * P); fill(D.cl, 2 * SFX_NHAND); fill(D.cr, 2 * SFX_NHAND);
    fill(D.pm, SFX_POSE); fill(D.jr, (size_t)SFX_J * V);
    for (int j = 0; j < SFX_J; ++j) for (int v = 0; v < V; ++v) if ((j + v) % 3) D.jr[(size_t)j * V + v] = 0.f;    // sparse regressor
    D.W.assign((size_t)V * SFX_J, 0.f);
    for (int v = 0; v < V; ++v) set_weights(D, v, 1 + v % 4);
    set_weights(D, 5, 10);                              // one vertex with more than SFX_NW nonzero weights,
    set_weights(D, 20, SFX_NW);                         // one that just fits (both carry items)
    D.par.resize(SFX_J); for (int j = 0; j < SFX_J; ++j) D.par[j] = j ? (j - 1) / 2 : -1;
    for (int f = 0; f < F; ++f) { D.faces.push_back(f % V); D.faces.push_back((f * 3 + 1) % V); D.faces.push_back((f * 5 + 2) % V); }
    D.faces[0] = 5; D.faces[1] = 6; D.faces[2] = 36;    // face 0 carries the overflowing vertex and the last one
    D.extra = {5, 20, 36};
    D.lf = {3, 17, 17, 59}; fill(D.lb, NLMK * 3);
    D.df = {0, 11, 23, 42, 42, 58}; fill(D.db, ROWS * NDYN * 3);      // [ROWS][NDYN]
    // kinematic joints (one read twice), extra vertices, static landmarks (one vertex shared with an extra), dynamic last
    D.jm = {0, 7, 54, 7, 56, 55, 21, 58, 61, 57, 59, 63, 62};
    return D;
}

static std::vector<std::pair<int, float>> nonzeros(const Desc& D, int v) {
    std::vector<std::pair<int, float>> r;
    for (int j = 0; j < SFX_J; ++j) if (D.W[(size_t)v * SFX_J + j] != 0.f) r.push_back({j, D.W[(size_t)v * SFX_J + j]});
    return r;
}
static void check_packed(const Desc& D, int v, const int* wj, const float* ww) {
    const auto nz = nonzeros(D, v);
    CHECK((wj[0] == -1) == (nz.size() > SFX_NW));
    for (int s = 0; s < SFX_NW; ++s) {
        const bool live = s < (int)nz.size();
        if (!(s == 0 && nz.size() > SFX_NW)) CHECK(wj[s] == (live ? nz[s].first : 0));
        CHECK(ww[s] == (live ? nz[s].second : 0.f));
    }
}
// the per-joint lists (start[J+1] with offsets from `base`, items, weights) hold exactly W[vertex of item][j], items ascending
static void check_lists(const Desc& D, const int* start, int base, const int* it, const float* wv, int item0, const int* vids, int n) {
    std::vector<float> A((size_t)n * SFX_J, 0.f);
    for (int j = 0; j < SFX_J; ++j) {
        CHECK(start[j] <= start[j + 1]);
        for (int q = start[j] - base; q < start[j + 1] - base; ++q) {
            const int i = it[q] - item0;
            CHECK(i >= 0 && i < n && wv[q] != 0.f); if (i < 0 || i >= n) continue;
            if (q > start[j] - base) CHECK(it[q] > it[q - 1]);
            A[(size_t)i * SFX_J + j] += wv[q];
        }
    }
    for (int i = 0; i < n; ++i) for (int j = 0; j < SFX_J; ++j) CHECK(A[(size_t)i * SFX_J + j] == D.W[(size_t)vids[i] * SFX_J + j]);
}

static void check_tables(Desc& D, const ModelTables& T, bool expect_blocks) {
    const sfx_model_desc* d = D.get();
    const int* meta = T.meta.data();
    const int Vpad = 64, K = d->K;
    CHECK(T.Vpad == Vpad && (int)T.meta.size() == SFX_META_N && T.faces == D.faces);
    // blend-shape matrix: one matrix M(k, x), x = vertex * 3 + coordinate, zero outside [KD) x [3V)
    auto Mkx = [&](int k, size_t x) { return x >= (size_t)V * 3 || k >= S + P ? 0.f : k < S ? D.sd[x * S + k] : D.pd[x * P + k - S]; };
    CHECK(T.dirsT.size() == (size_t)V * 3 * SFX_KD_PAD && T.dirs_tiled.size() == (size_t)3 * Vpad * SFX_KD_PAD);
    for (size_t x = 0; x < (size_t)3 * Vpad; ++x)
        for (int k = 0; k < SFX_KD_PAD; ++k) {
            if (x < (size_t)V * 3) CHECK(T.dirsT[x * SFX_KD_PAD + k] == Mkx(k, x));
            CHECK(T.dirs_tiled[((x / 48) * SFX_KD_PAD + k) * 48 + x % 48] == Mkx(k, x));
#ifdef SFX_LAB
            CHECK(T.dirs.size() == T.dirs_tiled.size() && T.dirs[(size_t)k * 3 * Vpad + x] == Mkx(k, x));
#endif
        }
    // skinning weights
    CHECK(T.Wsp_j.size() == (size_t)V * SFX_NW && T.Wsp_w.size() == (size_t)V * SFX_NW);
    int n_over = 0;
    for (int v = 0; v < V; ++v) { check_packed(D, v, &T.Wsp_j[(size_t)v * SFX_NW], &T.Wsp_w[(size_t)v * SFX_NW]); n_over += T.Wsp_j[(size_t)v * SFX_NW] == -1; }
    CHECK(n_over >= 1 && n_over < V);
    {   // jv_*: the transpose of W
        std::vector<float> A((size_t)V * SFX_J, 0.f);
        CHECK(T.jv_start.size() == SFX_J + 1 && T.jv_start[0] == 0 && T.jv_start[SFX_J] == (int)T.jv_vid.size() && T.jv_vid.size() == T.jv_w.size());
        for (int j = 0; j < SFX_J; ++j)
            for (int q = T.jv_start[j]; q < T.jv_start[j + 1]; ++q) {
                CHECK(T.jv_vid[q] >= 0 && T.jv_vid[q] < V && T.jv_w[q] != 0.f && (q == T.jv_start[j] || T.jv_vid[q] > T.jv_vid[q - 1]));
                A[(size_t)T.jv_vid[q] * SFX_J + j] += T.jv_w[q];
            }
        CHECK(A == D.W);
    }
    {   // tj_*: W per 16-vertex tile over the tile's joints (ascending), count padded to a multiple of 4 with zero weights
        bool odd_count = false;
        CHECK((int)T.tj_n.size() == Vpad / 16 && T.tj_list.size() == (size_t)(Vpad / 16) * SFX_JPAD && T.tj_w.size() == T.tj_list.size() * 16);
        for (int t = 0; t < Vpad / 16; ++t) {
            std::set<int> used;
            for (int v = t * 16; v < std::min<int>(V, t * 16 + 16); ++v) for (auto& p : nonzeros(D, v)) used.insert(p.first);
            odd_count |= used.size() % 4 != 0;
            CHECK(T.tj_n[t] % 4 == 0 && T.tj_n[t] <= SFX_JPAD && T.tj_n[t] == (int)(used.size() + 3) / 4 * 4);
            int s = 0;
            for (int j : used) {
                CHECK(T.tj_list[(size_t)t * SFX_JPAD + s] == j);
                for (int q = 0; q < 16; ++q) CHECK(T.tj_w[((size_t)t * SFX_JPAD + s) * 16 + q] == (t * 16 + q < V ? D.W[(size_t)(t * 16 + q) * SFX_J + j] : 0.f));
                ++s;
            }
            for (; s < SFX_JPAD; ++s) {
                CHECK(T.tj_list[(size_t)t * SFX_JPAD + s] == 0);
                for (int q = 0; q < 16; ++q) CHECK(T.tj_w[((size_t)t * SFX_JPAD + s) * 16 + q] == 0.f);
            }
        }
        CHECK(odd_count);      // (the descriptor exercises the padding)
    }
    // folded joint regressor in double, and its rounding
    CHECK(T.J_template64.size() == SFX_J * 3 && T.J_dirs64.size() == (size_t)SFX_J * 3 * S && T.J_template.size() == SFX_J * 3 && T.J_dirs.size() == T.J_dirs64.size());
    for (int j = 0; j < SFX_J; ++j)
        for (int c = 0; c < 3; ++c) {
            double t = 0.0, e[S] = {};
            for (int v = 0; v < V; ++v) {
                const double w = D.jr[(size_t)j * V + v];
                t += w * D.vt[v * 3 + c];
                for (int l = 0; l < S; ++l) e[l] += w * D.sd[((size_t)v * 3 + c) * S + l];
            }
            CHECK(T.J_template64[j * 3 + c] == t && T.J_template[j * 3 + c] == (float)t);
            for (int l = 0; l < S; ++l) CHECK(T.J_dirs64[((size_t)j * 3 + c) * S + l] == e[l] && T.J_dirs[((size_t)j * 3 + c) * S + l] == (float)e[l]);
        }
    // tree blocks of meta
    {
        std::vector<int> depth(SFX_J, 0), seen(SFX_J, 0);
        int maxd = 0;
        for (int j = 1; j < SFX_J; ++j) { depth[j] = depth[D.par[j]] + 1; maxd = std::max(maxd, depth[j]); }
        int rounds = 0; while ((1 << rounds) < maxd + 1) ++rounds;
        CHECK(T.n_rounds == rounds && rounds <= SFX_MAX_ROUNDS);
        for (int j = 0; j < SFX_J; ++j) {
            CHECK(meta[MO_PAR + j] == (j ? D.par[j] : -1));
            const int lj = meta[MO_LJ + j];
            CHECK(lj >= 0 && lj < SFX_J && !seen[lj]++);
            if (j) CHECK(depth[meta[MO_LJ + j - 1]] < depth[lj] || (depth[meta[MO_LJ + j - 1]] == depth[lj] && meta[MO_LJ + j - 1] < lj));
            std::vector<int> kids; int sub = 1;
            for (int c = 0; c < SFX_J; ++c) {
                if (c && D.par[c] == j) kids.push_back(c);
                int a = c; while (a > j) a = D.par[a];      // (parents precede children)
                if (c != j && a == j) {                     // c in the subtree of j: inside j's pre-order range
                    ++sub; CHECK(meta[MO_PRE + c] > meta[MO_PRE + j] && meta[MO_PRE + c] < meta[MO_PRE + j] + meta[MO_SUB + j]); }
            }
            CHECK(meta[MO_SUB + j] == sub && (kids.empty() || meta[MO_PRE + kids[0]] == meta[MO_PRE + j] + 1));
            CHECK(meta[MO_CS + j + 1] - meta[MO_CS + j] == (int)kids.size());
            for (size_t q = 0; q < kids.size(); ++q) CHECK(meta[MO_CL + meta[MO_CS + j] + q] == kids[q]);
            for (size_t q = 1; q < kids.size(); ++q) CHECK(meta[MO_PRE + kids[q]] == meta[MO_PRE + kids[q - 1]] + meta[MO_SUB + kids[q - 1]]);
            for (int k = 0; k < SFX_MAX_ROUNDS; ++k) {
                int a = j; for (int s = 0; s < (1 << k) && a >= 0; ++s) a = a ? D.par[a] : -1;
                CHECK(meta[MO_ANC + k * 56 + j] == (k < rounds ? a : 0));
            }
        }
        CHECK(meta[MO_CS] == 0 && meta[MO_PRE] == 0 && meta[MO_SUB] == SFX_J);
    }
    // mapped joints and items, from joint_map
    std::vector<int> ivid, idyn, ik; std::vector<float> iw;
    const int e0 = SFX_J, l0 = e0 + NEXTRA, d0 = l0 + NLMK;
    for (int k = 0; k < K; ++k) {
        const int s = D.jm[k], n = s < e0 ? 0 : s < l0 ? 1 : 3;
        CHECK(meta[MO_JT + k] == (s >= e0) && meta[MO_JS + k] == (s < e0 ? s : 0) && meta[MO_JN + k] == n && meta[MO_JI0 + k] == (n ? (int)ivid.size() : 0));
        for (int c = 0; c < n; ++c) {
            CHECK(meta[MO_IK + (int)ivid.size()] == k);
            ik.push_back(k);
            if (s < l0) { ivid.push_back(D.extra[s - e0]); iw.push_back(1.f); idyn.push_back(-1); }
            else if (s < d0) { ivid.push_back(D.faces[D.lf[s - l0] * 3 + c]); iw.push_back(D.lb[(s - l0) * 3 + c]); idyn.push_back(-1); }
            else { ivid.push_back(-1); iw.push_back(0.f); idyn.push_back((s - d0) * 3 + c); }
        }
    }
    for (int s = 0, n = 0; s <= SFX_J; ++s) {
        CHECK(meta[MO_SK0 + s] == n);
        for (int k = 0; k < K && s < SFX_J; ++k) if (D.jm[k] == s) CHECK(meta[MO_SKL + n++] == k);
    }
    const int ni = (int)ivid.size(), nd = 3 * NDYN, ns = ni - nd;
    CHECK(T.n_items == ni && T.n_static_items == ns && T.n_dyn_items == nd && T.item_vid == ivid && T.item_w == iw);
    CHECK(T.item_vt.size() == (size_t)ni * 3 && T.item_wj.size() == (size_t)ni * SFX_NW && T.item_ww.size() == (size_t)ni * SFX_NW && (int)T.item_uslot.size() == ni);
    int item_over = 0;
    for (int i = 0; i < ni; ++i) {
        CHECK((idyn[i] >= 0) == (i >= ns));
        for (int c = 0; c < 3; ++c) CHECK(T.item_vt[i * 3 + c] == (i < ns ? D.vt[ivid[i] * 3 + c] : 0.f));
        if (i < ns) { check_packed(D, ivid[i], &T.item_wj[(size_t)i * SFX_NW], &T.item_ww[(size_t)i * SFX_NW]); item_over += T.item_wj[(size_t)i * SFX_NW] == -1; }
        else for (int s = 0; s < SFX_NW; ++s) CHECK(T.item_wj[(size_t)i * SFX_NW + s] == 0 && T.item_ww[(size_t)i * SFX_NW + s] == 0.f);
    }
    CHECK(item_over >= 1);
    CHECK(T.sj_start.size() == SFX_J + 1 && T.sj_start[0] == 0 && T.n_sj == (int)T.sj_item.size() && T.sj_start[SFX_J] == T.n_sj && T.sj_w.size() == T.sj_item.size());
    check_lists(D, T.sj_start.data(), 0, T.sj_item.data(), T.sj_w.data(), 0, ivid.data(), ns);
    // per LUT row: the dynamic items' vertices, weights, template rows, packed skinning weights, per-joint lists
    CHECK(T.dynp_vid.size() == (size_t)ROWS * nd && T.dynp_w.size() == T.dynp_vid.size() && T.dynp_vt.size() == T.dynp_vid.size() * 3);
    CHECK(T.dynp_wj.size() == (size_t)ROWS * nd * SFX_NW && T.dynp_ww.size() == T.dynp_wj.size() && T.dynp_ji.size() == T.dynp_wj.size() && T.dynp_jw.size() == T.dynp_wj.size());
    CHECK(T.dj_start.size() == (size_t)ROWS * (SFX_J + 1) && T.dj_item.size() == T.dj_w.size() && T.dynp_us.size() == T.dynp_vid.size());
    CHECK(T.dynp_js.size() == (expect_blocks ? T.dj_start.size() : 0));
    int dyn_over = 0, rows_over = 0, rows_after_over = 0;
    for (int row = 0; row < ROWS; ++row) {
        std::vector<int> vids;
        for (int q = 0; q < nd; ++q) {
            const int l = idyn[ns + q] / 3, c = idyn[ns + q] % 3, v = D.faces[D.df[row * NDYN + l] * 3 + c];
            const size_t o = (size_t)row * nd + q;
            vids.push_back(v);
            // the forward part of every row's block is filled, the rows of and after an overflowing one included
            CHECK(T.dynp_vid[o] == v && T.dynp_w[o] == D.db[(row * NDYN + l) * 3 + c]);
            for (int e = 0; e < 3; ++e) CHECK(T.dynp_vt[o * 3 + e] == D.vt[v * 3 + e]);
            check_packed(D, v, &T.dynp_wj[o * SFX_NW], &T.dynp_ww[o * SFX_NW]); dyn_over += T.dynp_wj[o * SFX_NW] == -1;
        }
        const int* st = &T.dj_start[(size_t)row * (SFX_J + 1)];
        CHECK(st[0] == (row ? st[-1] : 0) && (row + 1 < ROWS || st[SFX_J] == (int)T.dj_item.size()));
        check_lists(D, st, 0, T.dj_item.data(), T.dj_w.data(), ns, vids.data(), nd);
        rows_after_over += rows_over > 0;
        rows_over += st[SFX_J] - st[0] > nd * SFX_NW;
        if (T.dynp_js.empty()) {        // row overflow: the per-joint part of the blocks is dropped (dj_* serve), left zero
            for (int q = 0; q < nd * SFX_NW; ++q) CHECK(T.dynp_ji[(size_t)row * nd * SFX_NW + q] == 0 && T.dynp_jw[(size_t)row * nd * SFX_NW + q] == 0.f);
            continue;
        }
        const int* js = &T.dynp_js[(size_t)row * (SFX_J + 1)];
        for (int j = 0; j <= SFX_J; ++j) CHECK(js[j] == st[j] - st[0]);
        CHECK(js[SFX_J] <= nd * SFX_NW);
        check_lists(D, js, 0, &T.dynp_ji[(size_t)row * nd * SFX_NW], &T.dynp_jw[(size_t)row * nd * SFX_NW], ns, vids.data(), nd);
    }
    CHECK(dyn_over >= 1 && (rows_over == 0) == expect_blocks);
    CHECK(expect_blocks || rows_after_over >= 1);      // (the overflow descriptor has a row after the overflowing one)
    // export slots
    std::set<int> uniq(ivid.begin(), ivid.begin() + ns), slots; uniq.insert(T.dynp_vid.begin(), T.dynp_vid.end());
    CHECK((int)T.vslot.size() == Vpad && T.n_uniq == (int)uniq.size());
    for (int v = 0; v < Vpad; ++v) {
        CHECK((T.vslot[v] >= 0) == (uniq.count(v) == 1) && T.vslot[v] < T.n_uniq);
        if (T.vslot[v] >= 0) CHECK(slots.insert(T.vslot[v]).second);
    }
    for (int i = 0; i < ni; ++i) CHECK(T.item_uslot[i] == (i < ns ? T.vslot[ivid[i]] : -1));
    for (size_t o = 0; o < T.dynp_vid.size(); ++o) CHECK(T.dynp_us[o] == T.vslot[T.dynp_vid[o]]);
}

static void check_refusal(const char* what, Desc& D, const char* msg) {
    ModelTables T; g_msg[0] = 0;
    const int rc = sfx_build_model_tables(D.get(), &T);
    printf("refusal (%s): rc %d, \"%s\"\n", what, rc, g_msg);
    CHECK(rc == -1 && std::string(g_msg).find(msg) != std::string::npos);
    CHECK(T.meta.empty() && T.dirsT.empty() && T.item_vid.empty() && T.faces.empty() && T.Vpad == 0 && T.n_items == 0);    // no table built
}

int main() {
    {
        Desc D = make_desc(); ModelTables T;
        CHECK(sfx_build_model_tables(D.get(), &T) == 0);
        check_tables(D, T, true);
        printf("descriptor 1: V %d Vpad %d items %d (static %d, dynamic %d) n_uniq %d n_sj %d rounds %d; %d checks\n", V, T.Vpad, T.n_items,
               T.n_static_items, T.n_dyn_items, T.n_uniq, T.n_sj, T.n_rounds, g_checks);
    }
    for (int last = 6; last <= 7; ++last) {     // LUT row 1 (vertices 23 33 6 | 5 16 27) with exactly nd * SFX_NW = 48 adjoint entries
        Desc D = make_desc();                   // still fits its block; with one more there is no dynp_js and dj_* serve
        for (int v : {23, 33, 6, 16}) set_weights(D, v, SFX_NW);
        set_weights(D, 27, last);               // (vertex 5 has 10)
        ModelTables T;
        CHECK(sfx_build_model_tables(D.get(), &T) == 0);
        check_tables(D, T, last == 6);
        printf("descriptor %d: row 1 has %d adjoint entries, dynp_js %s; %d checks\n", last - 4, T.dj_start[2 * (SFX_J + 1)] - T.dj_start[SFX_J + 1],
               T.dynp_js.empty() ? "absent (row overflow)" : "present", g_checks);
    }
    { Desc D = make_desc(); D.par[3] = 5; check_refusal("tree order", D, "parents must be topologically ordered"); }
    { Desc D = make_desc(); for (int j = 1; j < SFX_J; ++j) D.par[j] = j - 1; check_refusal("tree depth", D, "tree too deep"); }
    { Desc D = make_desc(); D.jm[2] = SFX_J + NEXTRA + NLMK + NDYN; check_refusal("joint_map range", D, "joint_map[2]=64 out of range [0,64)"); }
    { Desc D = make_desc(); D.jm[0] = -1; check_refusal("joint_map negative", D, "out of range"); }
    { Desc D = make_desc(); D.jm.assign(81, SFX_J + NEXTRA); check_refusal("item count", D, "too many vertex items"); }
    {   Desc D = make_desc(); D.df.assign(ROWS * 22, 0); D.db.assign(ROWS * 22 * 3, 0.25f); D.jm.clear();
        for (int l = 0; l < 22; ++l) D.jm.push_back(SFX_J + NEXTRA + NLMK + l);
        check_refusal("dynamic-item count", D, "too many dynamic-contour items (66 > 64)"); }
    { Desc D = make_desc(); std::swap(D.jm[9], D.jm[11]); check_refusal("dynamic before static", D, "dynamic items must trail the static ones"); }
    printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
