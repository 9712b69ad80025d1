// model.hip -- sfx_model_*: the model constants resident in HBM (tables built on the host by model_tables.h), the part table of
// the interpenetration term and the VPoser decoder's weights.
#include "host.h"
#include "../model_tables.h"
#include "../vposer_pack.h"

#include <memory>

extern "C" int sfx_model_create(const sfx_model_desc* d, sfx_model** out) {
    if (!d || !out) { sfx_set_error("null argument"); return -1; }
    if (d->J != SFX_J) { sfx_set_error("only J=55 (SMPL-X) is supported, got %d", d->J); return -1; }
    const int V = d->V, S = d->num_betas + d->num_expr, KD = S + 9 * (d->J - 1);
    if (KD > SFX_KD_PAD) { sfx_set_error("blend-shape depth %d unsupported", KD); return -1; }
    if (d->K > SFX_MAX_K) { sfx_set_error("K=%d > %d", d->K, SFX_MAX_K); return -1; }
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
        sfx_set_error("no HIP device: libsfx has no CPU fallback"); return -3;
    }
    ModelTables T;
    if (int rc = sfx_build_model_tables(d, &T)) return rc;      // every refusal: before the first device allocation
    std::unique_ptr<sfx_model> m(new sfx_model());
    DevModel& M = m->M;
    DevAlloc& mem = m->mem;
    m->NB = d->num_betas; m->NE = d->num_expr; m->NPCA = d->num_pca;
    M.V = V; M.S = S; M.K = d->K; M.n_dyn = d->n_dyn; M.Vpad = T.Vpad; M.n_rounds = T.n_rounds;
    M.n_items = T.n_items; M.n_static_items = T.n_static_items; M.n_uniq = T.n_uniq; M.n_sj = T.n_sj; M.n_dyn_items = T.n_dyn_items;
    M.v_template = mem.up(d->v_template, (size_t)V * 3);
#ifdef SFX_LAB
    M.dirs = mem.up(T.dirs);
#endif
    M.dirsT = mem.up(T.dirsT); M.dirs_tiled = mem.up(T.dirs_tiled);
    M.Wsp_j = mem.up(T.Wsp_j); M.Wsp_w = mem.up(T.Wsp_w);
    M.jv_start = mem.up(T.jv_start); M.jv_vid = mem.up(T.jv_vid); M.jv_w = mem.up(T.jv_w);
    M.W = mem.up(d->lbs_weights, (size_t)V * SFX_J);
    M.tj_n = mem.up(T.tj_n); M.tj_list = mem.up(T.tj_list); M.tj_w = mem.up(T.tj_w);
    M.J_template = mem.up(T.J_template); M.J_dirs = mem.up(T.J_dirs);
    M.J_template64 = mem.up(T.J_template64); M.J_dirs64 = mem.up(T.J_dirs64);
    M.comp_l = mem.up(d->hands_comp_l, (size_t)d->num_pca * SFX_NHAND); M.comp_r = mem.up(d->hands_comp_r, (size_t)d->num_pca * SFX_NHAND);
    M.pose_mean = mem.up(d->pose_mean, SFX_POSE);
    M.sj_start = mem.up(T.sj_start); M.sj_item = mem.up(T.sj_item); M.sj_w = mem.up(T.sj_w);
    M.dj_start = mem.up(T.dj_start); M.dj_item = mem.up(T.dj_item); M.dj_w = mem.up(T.dj_w);
    M.dynp_vid = mem.up(T.dynp_vid); M.dynp_w = mem.up(T.dynp_w); M.dynp_vt = mem.up(T.dynp_vt);
    M.dynp_wj = mem.up(T.dynp_wj); M.dynp_ww = mem.up(T.dynp_ww);
    M.dynp_js = T.dynp_js.empty() ? nullptr : mem.up(T.dynp_js);
    M.dynp_ji = mem.up(T.dynp_ji); M.dynp_jw = mem.up(T.dynp_jw);
    M.item_vid = mem.up(T.item_vid); M.item_w = mem.up(T.item_w);
    M.item_vt = mem.up(T.item_vt); M.item_wj = mem.up(T.item_wj); M.item_ww = mem.up(T.item_ww);
    M.dynp_us = T.dynp_us.empty() ? nullptr : mem.up(T.dynp_us);
    M.vslot = mem.up(T.vslot); M.item_uslot = mem.up(T.item_uslot); M.uniq_dirs = mem.up(T.uniq_dirs);
    M.meta = mem.up(T.meta);
    m->tile_key = mem.up(T.tile_key); m->tile_rest = mem.up(T.tile_rest);
    m->n_key = (int)T.tile_key.size(); m->n_rest = (int)T.tile_rest.size();
    m->meta_host = std::move(T.meta); m->faces_host = std::move(T.faces);
    if (mem.failed) { (void)hipGetLastError(); sfx_set_error("out of device memory (model constants)"); return -2; }
    if (hipDeviceSynchronize() != hipSuccess) { sfx_set_error("model upload failed"); return -2; }
    *out = m.release();
    return 0;
}

extern "C" void sfx_model_destroy(sfx_model* m) { delete m; }

extern "C" int sfx_model_set_parts(sfx_model* m, const int32_t* segm, const int32_t* parents, const int32_t* ign_pairs,
                                   int32_t n_ign) {
    if (!m) { sfx_set_error("null argument"); return -1; }
    ++m->parts_gen; m->pen_idle.drop();
    if (!segm && !parents) {        // no FilterFaces module (fit_single_frame.py:316 without part_segm_fn): no pair is filtered by part
        m->segm_host.clear(); m->parents_host.clear(); m->ign_host.clear();
        return 0;
    }
    if (!segm || !parents) { sfx_set_error("null argument"); return -1; }
    const size_t F = m->faces_host.size() / 3;
    m->segm_host.assign(segm, segm + F);
    m->parents_host.assign(parents, parents + F);
    m->ign_host.clear();
    if (ign_pairs && n_ign > 0) m->ign_host.assign(ign_pairs, ign_pairs + (size_t)2 * n_ign);
    return 0;
}

extern "C" int sfx_model_set_vposer(sfx_model* m, int32_t latent, int32_t hidden, const float* w1, const float* b1,
                                    const float* w2, const float* b2, const float* w3, const float* b3) {
    if (!m) { sfx_set_error("null model"); return -1; }
    if (!vposer_shape_ok(latent, hidden)) return -1;
    auto v = [](const float* p, size_t n) { return std::vector<float>(p, p + n); };
    const int H = hidden, L = latent;
    VposerPack P;
    vposer_pack(L, H, w1, w2, w3, P);
    m->M.vp_latent = latent; m->M.vp_hidden = hidden;
    m->M.vp_w1 = m->mem.up(v(w1, (size_t)H * L)); m->M.vp_b1 = m->mem.up(v(b1, H));
    m->M.vp_w2 = m->mem.up(v(w2, (size_t)H * H)); m->M.vp_b2 = m->mem.up(v(b2, H));
    m->M.vp_w3 = m->mem.up(v(w3, (size_t)126 * H)); m->M.vp_b3 = m->mem.up(v(b3, 126));
    m->M.vp_w1T = m->mem.up(P.w1T); m->M.vp_w2T = m->mem.up(P.w2T); m->M.vp_w3T = m->mem.up(P.w3T);
    if (m->mem.failed) { (void)hipGetLastError(); m->M.vp_latent = 0; sfx_set_error("out of device memory (VPoser weights)"); return -2; }
    if (m->fwd) { sfx_batch_destroy(m->fwd); m->fwd = nullptr; }
    return 0;
}
