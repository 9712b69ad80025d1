// model_tables.h -- every derived constant table of a model, built from its descriptor on the host: no HIP call, no device
// memory.  sfx_model_create (host/model.hip) uploads the result; tests/model_tables_check.cpp checks it on the CPU.  The arrays a model
// takes over unchanged (v_template, lbs_weights, hand components, pose_mean) are uploaded straight from the descriptor.
#pragma once
#include "../../include/sfx.h"
#include "sfx_internal.h"
#include <algorithm>
#include <cstring>
#include <vector>

struct ModelTables {      // members named after the DevModel pointers they become; layouts documented there
    int Vpad = 0, n_rounds = 0, n_items = 0, n_static_items = 0, n_uniq = 0, n_sj = 0, n_dyn_items = 0;
#ifdef SFX_LAB
    std::vector<float> dirs;
#endif
    std::vector<float> dirs_tiled, dirsT, uniq_dirs, tj_w, jv_w, Wsp_w, J_template, J_dirs, item_w, item_vt, item_ww, sj_w, dj_w;
    std::vector<float> dynp_w, dynp_vt, dynp_ww, dynp_jw;
    std::vector<double> J_template64, J_dirs64;
    std::vector<int> tj_n, tj_list, jv_start, jv_vid, Wsp_j, vslot, uniq_vid, item_uslot, item_vid, item_wj, sj_start, sj_item;
    std::vector<int> dj_start, dj_item, dynp_vid, dynp_wj, dynp_js, dynp_ji, dynp_us;     // dynp_js empty: the rows do not fit
    std::vector<int> meta;        // [SFX_META_N] the MO_* blocks: tree, mapped joints, item owners
    std::vector<int> faces;       // host copy for the collision handle
    // the dense GEMM's 16-vertex tiles (ceil(V / 16) of them) in two ascending lists: tile_key holds the tiles with at least
    // one exported vertex (vslot >= 0: what the per-frame kernel reads back as uvp), tile_rest every other tile
    std::vector<int> tile_key, tile_rest;
};

// The nonzero weights of vertex v in ascending joint order, packed into SFX_NW slots (pad: j = 0, w = 0).  A row with more
// nonzeros than that is flagged by j[0] = -1: the kernels then read the vertex's full row of lbs_weights (same order).
static inline void sfx_pack_weights(const float* W, int v, int* wj, float* ww) {
    int n = 0;
    for (int j = 0; j < SFX_J; ++j) {
        const float w = W[(size_t)v * SFX_J + j];
        if (w == 0.f) continue;
        if (n < SFX_NW) { wj[n] = j; ww[n] = w; }
        ++n;
    }
    if (n > SFX_NW) wj[0] = -1;
}
// vertex of corner c of dynamic-contour landmark l in LUT row `row`
static inline int sfx_dyn_vertex(const sfx_model_desc* d, int row, int l, int c) {
    return d->faces[(size_t)d->dyn_lmk_faces_idx[(size_t)row * d->n_dyn + l] * 3 + c];
}

// Expects what sfx_model_create has checked (J = SFX_J, KD <= SFX_KD_PAD, K <= SFX_MAX_K).  Returns 0 and fills *out, or
// refuses with -1 and a message (sfx_set_error), leaving *out untouched: every refusal precedes the large tables.
static inline int sfx_build_model_tables(const sfx_model_desc* d, ModelTables* out) {
    ModelTables T;
    const int V = d->V, S = d->num_betas + d->num_expr, P = 9 * (SFX_J - 1), K = d->K;
    const float* W = d->lbs_weights;
    T.Vpad = ((V + 31) / 32) * 32;
    T.meta.assign(SFX_META_N, 0);
    int* meta = T.meta.data();
    // kinematic tree: depth levels, child lists
    std::vector<int> par(d->parents, d->parents + SFX_J), depth(SFX_J, 0);
    par[0] = -1;
    int maxd = 0;
    for (int j = 1; j < SFX_J; ++j) {
        if (par[j] < 0 || par[j] >= j) { sfx_set_error("parents must be topologically ordered"); return -1; }
        depth[j] = depth[par[j]] + 1; maxd = std::max(maxd, depth[j]);
    }
    while ((1 << T.n_rounds) <= maxd) ++T.n_rounds;     // pointer-jumping rounds: ceil(log2(levels))
    if (maxd + 1 > SFX_MAX_LEVELS || T.n_rounds > SFX_MAX_ROUNDS) { sfx_set_error("tree too deep"); return -1; }
    int *cs = meta + MO_CS, *cl = meta + MO_CL;
    for (int j = 0; j < SFX_J; ++j) meta[MO_PAR + j] = par[j];
    for (int l = 0, n = 0; l <= maxd; ++l) for (int j = 0; j < SFX_J; ++j) if (depth[j] == l) meta[MO_LJ + n++] = j;
    for (int j = 0, n = 0; j <= SFX_J; ++j) { cs[j] = n; for (int c = j + 1; c < SFX_J; ++c) if (par[c] == j) cl[n++] = c; }
    {   // DFS pre-order (children in ascending joint order) and subtree sizes: the adjoint of the chain sums over subtrees,
        // which are contiguous pre-order ranges
        std::vector<int> stack{0};
        for (int pos = 0; !stack.empty();) {
            const int j = stack.back(); stack.pop_back();
            meta[MO_PRE + j] = pos++;
            for (int q = cs[j + 1] - 1; q >= cs[j]; --q) stack.push_back(cl[q]);
        }
        for (int j = 0; j < SFX_J; ++j) meta[MO_SUB + j] = 1;
        for (int j = SFX_J - 1; j > 0; --j) meta[MO_SUB + par[j]] += meta[MO_SUB + j];
        std::vector<int> anc(par), nxt(SFX_J);      // 2^k-th ancestors for the pointer-jumping evaluation of the chain
        for (int k = 0; k < T.n_rounds; ++k) {
            for (int j = 0; j < SFX_J; ++j) { meta[MO_ANC + k * 56 + j] = anc[j]; nxt[j] = anc[j] < 0 ? -1 : anc[anc[j]]; }
            anc = nxt;
        }
    }
    // mapped joints -> kinematic joints / vertex items (an item: one weighted vertex; a landmark is three)
    std::vector<int> idyn, ik;       // per item: -1 or (landmark * 3 + corner) of the dynamic LUT; owning mapped joint
    const int e0 = SFX_J, l0 = e0 + d->n_extra, d0 = l0 + d->n_lmk, end = d0 + d->n_dyn;
    for (int k = 0; k < K; ++k) {
        const int s = d->joint_map[k];
        if (s < 0 || s >= end) { sfx_set_error("joint_map[%d]=%d out of range [0,%d)", k, s, end); return -1; }
        if (s < e0) { meta[MO_JS + k] = s; continue; }
        meta[MO_JT + k] = 1; meta[MO_JI0 + k] = (int)ik.size(); meta[MO_JN + k] = s < l0 ? 1 : 3;
        auto item = [&](int vid, float w, int dyn) { T.item_vid.push_back(vid); T.item_w.push_back(w); idyn.push_back(dyn); ik.push_back(k); };
        if (s < l0) item(d->extra_vertex_ids[s - e0], 1.f, -1);                 // an extra vertex
        else if (s < d0)                                                        // a static landmark: the corners of its face
            for (int c = 0, l = s - l0; c < 3; ++c) item(d->faces[(size_t)d->lmk_faces_idx[l] * 3 + c], d->lmk_bary[l * 3 + c], -1);
        else                                                                    // a dynamic landmark: vertices come per LUT row
            for (int c = 0, l = s - d0; c < 3; ++c) item(-1, 0.f, l * 3 + c);
    }
    const int ni = T.n_items = (int)ik.size();
    if (ni > SFX_MAX_ITEMS) { sfx_set_error("too many vertex items"); return -1; }
    for (int i = 0; i < ni; ++i) (idyn[i] < 0 ? T.n_static_items : T.n_dyn_items) += 1;
    const int ns = T.n_static_items, nd = T.n_dyn_items, rows = nd ? d->n_dyn_rows : 0;
    if (nd > SFX_MAX_DYN) { sfx_set_error("too many dynamic-contour items (%d > %d)", nd, SFX_MAX_DYN); return -1; }
    for (int i = 0; i + 1 < ni; ++i)
        if (idyn[i] >= 0 && idyn[i + 1] < 0) { sfx_set_error("internal: dynamic items must trail the static ones"); return -1; }
    for (int i = 0; i < ni; ++i) meta[MO_IK + i] = ik[i];
    for (int s = 0, n = 0; s <= SFX_J; ++s) {           // CSR: mapped joints that read kinematic joint s
        meta[MO_SK0 + s] = n;
        for (int k = 0; k < K; ++k) if (!meta[MO_JT + k] && meta[MO_JS + k] == s) meta[MO_SKL + n++] = k;
    }
    // per-joint adjoint lists of (item, skinning weight) over n items on vertices vids[]; offsets absolute into it / wv
    auto by_joint = [&](const int* vids, int item0, int n, std::vector<int>& start, std::vector<int>& it, std::vector<float>& wv) {
        for (int j = 0; j <= SFX_J; ++j) {
            start.push_back((int)it.size());
            for (int q = 0; q < n && j < SFX_J; ++q) {
                const float w = W[(size_t)vids[q] * SFX_J + j];
                if (w != 0.f) { it.push_back(item0 + q); wv.push_back(w); }
            }
        }
    };
    by_joint(T.item_vid.data(), 0, ns, T.sj_start, T.sj_item, T.sj_w);
    T.n_sj = (int)T.sj_item.size();
    // template rows and packed skinning weights gathered per static item: the per-frame kernels fetch them in ONE round trip
    T.item_vt.assign((size_t)ni * 3, 0.f); T.item_wj.assign((size_t)ni * SFX_NW, 0); T.item_ww.assign((size_t)ni * SFX_NW, 0.f);
    for (int i = 0; i < ns; ++i) {
        std::memcpy(&T.item_vt[(size_t)i * 3], d->v_template + (size_t)T.item_vid[i] * 3, 3 * sizeof(float));
        sfx_pack_weights(W, T.item_vid[i], &T.item_wj[(size_t)i * SFX_NW], &T.item_ww[(size_t)i * SFX_NW]);
    }
    // everything about the dynamic items that depends on the LUT row, in one fixed-size block per row (closure_body fetches a
    // block asynchronously), and the rows' per-joint lists twice: dj_* back to back, dynp_j* per block when every row fits
    const size_t RB = (size_t)nd * SFX_NW;
    T.dynp_vid.assign((size_t)rows * nd, 0); T.dynp_w.assign((size_t)rows * nd, 0.f); T.dynp_vt.assign((size_t)rows * nd * 3, 0.f);
    T.dynp_wj.assign(rows * RB, 0); T.dynp_ww.assign(rows * RB, 0.f);
    T.dynp_js.assign((size_t)rows * (SFX_J + 1), 0); T.dynp_ji.assign(rows * RB, 0); T.dynp_jw.assign(rows * RB, 0.f);
    // Row overflow: a row whose vertices carry more than nd * SFX_NW weights in all does not fit the per-joint part of its
    // block.  Then no row's dynp_js / dynp_ji / dynp_jw is used (dynp_js is dropped, closure_body walks dj_* instead); the
    // forward part of EVERY row's block (dynp_vid / w / vt / wj / ww / us) is filled regardless: closure_body reads it for
    // whatever row the head pose selects.
    bool fit = true;
    std::vector<int> vids(nd);
    for (int row = 0; row < rows; ++row) {
        for (int q = 0; q < nd; ++q) vids[q] = sfx_dyn_vertex(d, row, idyn[ns + q] / 3, idyn[ns + q] % 3);
        by_joint(vids.data(), ns, nd, T.dj_start, T.dj_item, T.dj_w);
        for (int q = 0; q < nd; ++q) {
            const int l = idyn[ns + q] / 3, c = idyn[ns + q] % 3, v = vids[q];
            const size_t o = (size_t)row * nd + q;
            T.dynp_vid[o] = v; T.dynp_w[o] = d->dyn_lmk_bary[((size_t)row * d->n_dyn + l) * 3 + c];
            std::memcpy(&T.dynp_vt[o * 3], d->v_template + (size_t)v * 3, 3 * sizeof(float));
            sfx_pack_weights(W, v, &T.dynp_wj[o * SFX_NW], &T.dynp_ww[o * SFX_NW]);
        }
        if (!fit) continue;
        const int* st = &T.dj_start[(size_t)row * (SFX_J + 1)];
        const size_t n_row = st[SFX_J] - st[0];
        if (n_row > RB) { fit = false; continue; }      // (> SFX_NW weights per vertex on average: the closure reads dj_*)
        for (int j = 0; j <= SFX_J; ++j) T.dynp_js[(size_t)row * (SFX_J + 1) + j] = st[j] - st[0];
        std::copy_n(&T.dj_item[st[0]], n_row, &T.dynp_ji[row * RB]); std::copy_n(&T.dj_w[st[0]], n_row, &T.dynp_jw[row * RB]);
    }
    if (!fit) { T.dynp_js.clear(); T.dynp_ji.assign(rows * RB, 0); T.dynp_jw.assign(rows * RB, 0.f); }
    // export slots: distinct vertices of the static items and of every vertex a dynamic item can land on (all LUT rows) -- the
    // dense GEMM hands their blend offsets to the per-frame kernel, which then streams no blend-shape row forward
    T.vslot.assign(T.Vpad, -1); T.item_uslot.assign(ni, -1); T.dynp_us.resize(T.dynp_vid.size());
    auto slot_of = [&](int v) { if (T.vslot[v] < 0) { T.vslot[v] = T.n_uniq++; T.uniq_vid.push_back(v); } return T.vslot[v]; };
    for (int i = 0; i < ns; ++i) T.item_uslot[i] = slot_of(T.item_vid[i]);
    for (size_t o = 0; o < T.dynp_vid.size(); ++o) T.dynp_us[o] = slot_of(T.dynp_vid[o]);
    for (int t = 0; t < (V + 15) / 16; ++t) {           // (vslot has Vpad >= 16 ceil(V / 16) entries, -1 beyond V)
        bool key = false;
        for (int q = 0; q < 16 && !key; ++q) key = T.vslot[(size_t)t * 16 + q] >= 0;
        (key ? T.tile_key : T.tile_rest).push_back(t);
    }
    // blend-shape matrix (shape | pose directions, zero beyond KD), vertex-major [V][3][KD_PAD] and tile-major
    // [Vpad/16][KD_PAD][16 vertices x 3 coordinates] (the lab build: and k-major [KD_PAD][3*Vpad])
    const size_t LD = (size_t)3 * T.Vpad;
    T.dirsT.assign((size_t)V * 3 * SFX_KD_PAD, 0.f); T.dirs_tiled.assign(LD * SFX_KD_PAD, 0.f);
#ifdef SFX_LAB
    T.dirs.assign(LD * SFX_KD_PAD, 0.f);
#endif
    for (size_t x = 0; x < (size_t)V * 3; ++x) {        // x = vertex * 3 + coordinate
        float* row = &T.dirsT[x * SFX_KD_PAD];
        std::copy_n(d->shapedirs + x * S, S, row); std::copy_n(d->posedirs + x * P, P, row + S);
        for (int k = 0; k < S + P; ++k) {
            T.dirs_tiled[((x / 48) * SFX_KD_PAD + k) * 48 + x % 48] = row[k];
#ifdef SFX_LAB
            T.dirs[k * LD + x] = row[k];
#endif
        }
    }
    // the rows of the exported vertices once more, as the B operands of the per-frame kernel's own copy of the GEMM's chain
    // (closure_body.h self_blend_offsets): per unit = (tile of 16 export indices, coordinate) the 128 MFMA steps in the GEMM's K
    // order -- step s = 8 c + ks reads k = 32 SFX_DENSE_KCHUNK(c) + 4 ks + kq in lane kq * 16 + jl, column jl = export index
    // 16 tile + jl (the spare columns of a partial tile repeat the last vertex) -- laid out [unit][s / 4][lane][s % 4]
    T.uniq_dirs.assign((size_t)((T.n_uniq + 15) / 16) * 3 * 128 * 64, 0.f);
    for (int unit = 0; unit < ((T.n_uniq + 15) / 16) * 3; ++unit)
        for (int s = 0; s < 128; ++s)
            for (int lane = 0; lane < 64; ++lane) {
                const int tile = unit / 3, co = unit % 3, jl = lane & 15, kq = lane >> 4;
                const int v = T.uniq_vid[std::min(tile * 16 + jl, T.n_uniq - 1)];
                const int k = SFX_DENSE_KC * SFX_DENSE_KCHUNK(s / 8) + 4 * (s % 8) + kq;
                T.uniq_dirs[(((size_t)unit * 32 + s / 4) * 64 + lane) * 4 + s % 4] = T.dirsT[((size_t)v * 3 + co) * SFX_KD_PAD + k];
            }
    // skinning weights: packed per vertex, transposed CSR, and per 16-vertex tile
    T.Wsp_j.assign((size_t)V * SFX_NW, 0); T.Wsp_w.assign((size_t)V * SFX_NW, 0.f);
    for (int v = 0; v < V; ++v) sfx_pack_weights(W, v, &T.Wsp_j[(size_t)v * SFX_NW], &T.Wsp_w[(size_t)v * SFX_NW]);
    for (int j = 0; j <= SFX_J; ++j) {
        T.jv_start.push_back((int)T.jv_vid.size());
        for (int v = 0; v < V && j < SFX_J; ++v) if (W[(size_t)v * SFX_J + j] != 0.f) { T.jv_vid.push_back(v); T.jv_w.push_back(W[(size_t)v * SFX_J + j]); }
    }
    const int nt = T.Vpad / 16;     // per tile: the joints with any nonzero weight (ascending), weights in MFMA B layout
    T.tj_n.assign(nt, 0); T.tj_list.assign((size_t)nt * SFX_JPAD, 0); T.tj_w.assign((size_t)nt * SFX_JPAD * 16, 0.f);
    for (int t = 0; t < nt; ++t) {
        int n = 0;
        for (int j = 0; j < SFX_J; ++j) {
            bool used = false;
            for (int q = 0; q < 16 && !used; ++q) { const int v = t * 16 + q; used = v < V && W[(size_t)v * SFX_J + j] != 0.f; }
            if (!used) continue;
            T.tj_list[(size_t)t * SFX_JPAD + n] = j;
            for (int q = 0; q < 16; ++q) { const int v = t * 16 + q; T.tj_w[((size_t)t * SFX_JPAD + n) * 16 + q] = v < V ? W[(size_t)v * SFX_J + j] : 0.f; }
            ++n;
        }
        T.tj_n[t] = ((n + 3) / 4) * 4;
    }
    // folded joint regressor: J = J_template + J_dirs . coeff   (J_regressor . v_shaped), accumulated in double
    T.J_template64.resize((size_t)SFX_J * 3); T.J_dirs64.resize((size_t)SFX_J * 3 * S);
    for (int j = 0; j < SFX_J; ++j) {
        std::vector<double> acc(3 + 3 * S, 0.0);
        const float* jr = d->J_regressor + (size_t)j * V;
        for (int v = 0; v < V; ++v) {
            const double w = jr[v];
            if (w == 0.0) continue;
            for (int c = 0; c < 3; ++c) {
                acc[c] += w * d->v_template[(size_t)v * 3 + c];
                const float* sd = d->shapedirs + ((size_t)v * 3 + c) * S;
                for (int l = 0; l < S; ++l) acc[3 + c * S + l] += w * sd[l];
            }
        }
        std::copy_n(acc.begin(), 3, &T.J_template64[(size_t)j * 3]); std::copy_n(acc.begin() + 3, 3 * S, &T.J_dirs64[(size_t)j * 3 * S]);
    }
    T.J_template.assign(T.J_template64.begin(), T.J_template64.end()); T.J_dirs.assign(T.J_dirs64.begin(), T.J_dirs64.end());
    T.faces.assign(d->faces, d->faces + (size_t)d->F * 3);
    *out = std::move(T);
    return 0;
}
