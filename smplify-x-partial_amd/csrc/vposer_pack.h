// vposer_pack.h -- host side of the VPoser-v1 decoder weights, shared by sfx_model_set_vposer (api.hip: the in-loop decoder of
// vposer.h) and sfx_vposer_create (vposer_batch.hip: the stand-alone operator): the one shape refusal and the transposed,
// padded copies the forward products stream ([in][out]).
#pragma once
#include "sfx_internal.h"

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
