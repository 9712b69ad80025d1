// vposer_pack.h -- host side of the VPoser-v1 decoder weights, shared by sfx_model_set_vposer (host/model.hip: the in-loop decoder of
// vposer.h) and sfx_vposer_create (vposer_batch.hip: the stand-alone operator): the one shape refusal and the transposed,
// padded copies the forward products stream ([in][out]).  Below them the encoder's side (sfx_vposer_encoder_create,
// vposer_encode.hip): its refusals, the batch norms folded into the linear layers, both orientations of every matrix.
#pragma once
#include "sfx_internal.h"
#include <cmath>

// hidden 512, latent a multiple of 4 and <= 60; a refusal sets the error text and needs no device
static inline bool vposer_shape_ok(int latent, int hidden) {
    if (hidden != 512 || latent < 4 || latent > 60 || latent % 4) {
        sfx_set_error("VPoser v1 decoder expected (hidden 512, latent a multiple of 4 <= 60), got %d/%d", latent, hidden); return false; }
    return true;
}

struct VposerPack { std::vector<float> w1T, w2T, w3T; };      // [L][512], [512][512], [512][128] (columns 126, 127 zero)

static inline void vposer_pack(int latent, int hidden, const float* w1, const float* w2, const float* w3, VposerPack& P) {
    const int H = hidden, L = latent;
    P.w1T.assign((size_t)L * H, 0.f); P.w2T.assign((size_t)H * H, 0.f); P.w3T.assign((size_t)H * 128, 0.f);
    for (int o = 0; o < H; ++o) for (int i = 0; i < L; ++i) P.w1T[(size_t)i * H + o] = w1[(size_t)o * L + i];
    for (int o = 0; o < H; ++o) for (int i = 0; i < H; ++i) P.w2T[(size_t)i * H + o] = w2[(size_t)o * H + i];
    for (int o = 0; o < 126; ++o) for (int i = 0; i < H; ++i) P.w3T[(size_t)i * 128 + o] = w3[(size_t)o * H + i];
}

// ---- encoder (sfx_vposer_encoder_create, vposer_encode.hip) ---------------------------------------------------------------
// bn1 -> fc1 (n_in -> 512) -> leaky_relu(0.2) -> bn2 -> fc2 (512 -> 512) -> leaky_relu(0.2) -> mu | logvar (512 -> L).
// Eval-mode batch norm is affine -- y = x * s + t with s = w / sqrt(var + 1e-5), t = b - mean * s -- and is folded into the linear
// layer that follows it, in double: W'[o][i] = fl32(W[o][i] * s[i]), b'[o] = fl32(b[o] + sum_i W[o][i] * t[i]) (ascending i).
// The device evaluates  front end -> W1' -> leaky -> W2' -> leaky -> head  with head = [mu ; logvar] as one [128]-row matrix:
// mu in rows 0 .. L-1, logvar in rows 64 .. 64+L-1, the rest zero.  Both orientations of the three matrices are packed, zero-
// padded (n_in 63 -> 64, 189 -> 192) so that no k step or column tile of the six products needs a bounds test.
// (VPE_EPS and the head layout VPE_HEAD / VPE_LV are defined here, not with the kernel's other VPE_* macros in vposer_encode.hip,
// because the packer below and the kernels must agree on them; the other files that include this header do not use them)
#define VPE_EPS 1e-5          // BatchNorm1d eps (BN_EPS of vposer.py)
#define VPE_HEAD 128          // rows of the head: mu from 0, logvar from VPE_LV
#define VPE_LV 64

struct VposerEncPack {
    int kin = 0;                                        // n_in padded: 64 | 192
    std::vector<float> w1T, w2T, whT;                   // [kin][512], [512][512], [512][128]: the forward products stream these
    std::vector<float> w1p, w2, wh;                     // [512][kin], [512][512], [128][512]: the backward's transposed products
    std::vector<float> b1, b2, bh;                      // [512], [512], [128]
};

// s, t of one batch-norm table; false (error text set) when var + eps <= 0 somewhere or a value is not finite
static inline bool vposer_bn_affine(const char* name, int n, const float* w, const float* b, const float* mean, const float* var,
                                    std::vector<double>& s, std::vector<double>& t) {
    s.resize(n); t.resize(n);
    for (int i = 0; i < n; ++i) {
        if (!std::isfinite(w[i]) || !std::isfinite(b[i]) || !std::isfinite(mean[i]) || !std::isfinite(var[i])) {
            sfx_set_error("VPoser encoder: %s has a non-finite value at %d", name, i); return false; }
        const double v = (double)var[i] + VPE_EPS;
        if (!(v > 0.0)) { sfx_set_error("VPoser encoder: %s running_var + 1e-5 <= 0 at %d (%g)", name, i, (double)var[i]); return false; }
        s[i] = (double)w[i] / std::sqrt(v);
        t[i] = (double)b[i] - (double)mean[i] * s[i];
    }
    return true;
}

// W [n_out][n_in], b [n_out] with the affine map (s, t) of its input folded in -> Wp [n_out][ld] (columns >= n_in stay zero),
// WT [ld rows][n_out] (rows >= n_in stay zero), bp [n_out]
static inline void vposer_fold(int n_out, int n_in, int ld, const float* W, const float* b, const std::vector<double>& s,
                               const std::vector<double>& t, std::vector<float>& Wp, std::vector<float>& WT, std::vector<float>& bp) {
    Wp.assign((size_t)n_out * ld, 0.f); WT.assign((size_t)ld * n_out, 0.f); bp.assign(n_out, 0.f);
    for (int o = 0; o < n_out; ++o) {
        double acc = (double)b[o];
        for (int i = 0; i < n_in; ++i) {
            const double w = (double)W[(size_t)o * n_in + i];
            const float f = (float)(w * s[i]);
            Wp[(size_t)o * ld + i] = f; WT[(size_t)i * n_out + o] = f;
            acc += w * t[i];
        }
        bp[o] = (float)acc;
    }
}

// every refusal of sfx_vposer_encoder_create but the null handle: sets the error text, needs no device
static inline bool vposer_pack_encoder(int latent, int hidden, int n_in,
                                       const float* bn1_w, const float* bn1_b, const float* bn1_mean, const float* bn1_var,
                                       const float* fc1_w, const float* fc1_b,
                                       const float* bn2_w, const float* bn2_b, const float* bn2_mean, const float* bn2_var,
                                       const float* fc2_w, const float* fc2_b,
                                       const float* mu_w, const float* mu_b, const float* logvar_w, const float* logvar_b,
                                       VposerEncPack& P) {
    if (!bn1_w || !bn1_b || !bn1_mean || !bn1_var || !fc1_w || !fc1_b || !bn2_w || !bn2_b || !bn2_mean || !bn2_var || !fc2_w ||
        !fc2_b || !mu_w || !mu_b || !logvar_w || !logvar_b) { sfx_set_error("null argument"); return false; }
    if (hidden != 512 || latent < 4 || latent > 60 || latent % 4) {
        sfx_set_error("VPoser v1 encoder expected (hidden 512, latent a multiple of 4 <= 60), got %d/%d", latent, hidden); return false; }
    if (n_in != 63 && n_in != 189) {
        sfx_set_error("VPoser v1 encoder expected 63 (axis-angle) or 189 (rotation matrix) inputs, got %d", n_in); return false; }
    const int H = hidden, L = latent;
    std::vector<double> s, t;
    P.kin = n_in == 63 ? 64 : 192;
    if (!vposer_bn_affine("bn1", n_in, bn1_w, bn1_b, bn1_mean, bn1_var, s, t)) return false;
    vposer_fold(H, n_in, P.kin, fc1_w, fc1_b, s, t, P.w1p, P.w1T, P.b1);
    if (!vposer_bn_affine("bn2", H, bn2_w, bn2_b, bn2_mean, bn2_var, s, t)) return false;
    vposer_fold(H, H, H, fc2_w, fc2_b, s, t, P.w2, P.w2T, P.b2);
    P.wh.assign((size_t)VPE_HEAD * H, 0.f); P.whT.assign((size_t)H * VPE_HEAD, 0.f); P.bh.assign(VPE_HEAD, 0.f);
    for (int half = 0; half < 2; ++half) {
        const float* w = half ? logvar_w : mu_w; const float* b = half ? logvar_b : mu_b;
        for (int o = 0; o < L; ++o) {
            const int r = half * VPE_LV + o;
            P.bh[r] = b[o];
            for (int i = 0; i < H; ++i) { P.wh[(size_t)r * H + i] = w[(size_t)o * H + i]; P.whT[(size_t)i * VPE_HEAD + r] = w[(size_t)o * H + i]; }
        }
    }
    return true;
}
