// CPU driver of the VPoser encoder's host packing (csrc/vposer_pack.h: vposer_pack_encoder).  Stand-alone: own main, no device.
//   vposer_pack_check IN OUT
// IN : int32 latent, hidden, n_in, then float32 bn1 (w, b, mean, var) [n_in], fc1_w [hidden][n_in], fc1_b [hidden], bn2 (w, b,
//      mean, var) [hidden], fc2_w [hidden][hidden], fc2_b, mu_w [latent][hidden], mu_b, logvar_w, logvar_b.
// OUT: int32 ok, kin, then (ok = 1) float32 w1T, w2T, whT, w1p, w2, wh, b1, b2, bh in the sizes of VposerEncPack; (ok = 0) the
//      error text.
// Built and run by tests/test_vposer_encode_host.py (host AddressSanitizer + UBSan), which compares with numpy.
#include "../smplify-x-partial_amd/csrc/vposer_pack.h"
#include <cstdarg>
#include <cstdio>
#include <cstring>

static char g_msg[512];
void sfx_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_msg, sizeof(g_msg), fmt, ap); va_end(ap); }

static bool rd(FILE* f, std::vector<float>& a, size_t n) { a.resize(n); return fread(a.data(), sizeof(float), n, f) == n; }
static void wr(FILE* f, const std::vector<float>& a) { fwrite(a.data(), sizeof(float), a.size(), f); }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    int32_t hdr[3];
    if (fread(hdr, sizeof(int32_t), 3, in) != 3) { fprintf(stderr, "short header\n"); return 2; }
    const size_t L = (size_t)hdr[0], H = (size_t)hdr[1], N = (size_t)hdr[2];
    std::vector<float> bn1[4], bn2[4], fc1_w, fc1_b, fc2_w, fc2_b, mu_w, mu_b, lv_w, lv_b;
    bool ok = true;
    for (auto& a : bn1) ok = ok && rd(in, a, N);
    ok = ok && rd(in, fc1_w, H * N) && rd(in, fc1_b, H);
    for (auto& a : bn2) ok = ok && rd(in, a, H);
    ok = ok && rd(in, fc2_w, H * H) && rd(in, fc2_b, H) && rd(in, mu_w, L * H) && rd(in, mu_b, L) && rd(in, lv_w, L * H) && rd(in, lv_b, L);
    fclose(in);
    if (!ok) { fprintf(stderr, "short input\n"); return 2; }
    VposerEncPack P;
    const bool good = vposer_pack_encoder(hdr[0], hdr[1], hdr[2], bn1[0].data(), bn1[1].data(), bn1[2].data(), bn1[3].data(),
                                          fc1_w.data(), fc1_b.data(), bn2[0].data(), bn2[1].data(), bn2[2].data(), bn2[3].data(),
                                          fc2_w.data(), fc2_b.data(), mu_w.data(), mu_b.data(), lv_w.data(), lv_b.data(), P);
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    const int32_t head[2] = {good ? 1 : 0, P.kin};
    fwrite(head, sizeof(int32_t), 2, out);
    if (good) { wr(out, P.w1T); wr(out, P.w2T); wr(out, P.whT); wr(out, P.w1p); wr(out, P.w2); wr(out, P.wh); wr(out, P.b1); wr(out, P.b2); wr(out, P.bh); }
    else fwrite(g_msg, 1, strlen(g_msg), out);
    fclose(out);
    printf("%s kin=%d %s\n", good ? "packed" : "refused", P.kin, good ? "" : g_msg);
    return 0;
}
