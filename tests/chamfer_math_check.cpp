// CPU check of the chamfer term's arithmetic and bookkeeping (csrc/chamfer_math.h): reads the cases tests/test_chamfer_host.py
// wrote to the file named first and writes what the header makes of them to the file named second.
//   in :  int32 n_pairs, n_rho, n_len, n_idx
//         n_pairs x 6 float32       (ax ay az bx by bz)                 -> float32 ch_dist2
//         n_rho x 4 float64         (s, rho, w, g; s, rho, w, g hold float32 values)
//                                                                       -> float64 ch_rho, ch_drho, ch_point_value, ch_coef
//         n_len x int32             list lengths                        -> int32 ch_seg_len
//         n_idx x { int32 nq, nt; nq x int32 idx }                      -> int32 off[nt + 1], list[nq] (padded with -1) by
//                                                                          ch_invert, list[nq] again by the device's way
// The device's way: the buckets are filled in a scrambled order of the queries (a cursor per bucket, as the kernel's integer
// atomics would), then every entry moves to its ch_rank.  Checked here: both ways give the same lists, every list is ascending,
// off is an exclusive scan.  Stand-alone: own main, no device.  Built and run with host AddressSanitizer + UBSan.
#include "../smplify-x-partial_amd/csrc/chamfer_math.h"
#include <cstdint>
#include <cstdio>
#include <vector>

static int g_fail = 0, g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { if (++g_fail <= 40) printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); } } while (0)

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
static void wr(FILE* f, const T* p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }

int main(int argc, char** argv) {
    if (argc != 3) { printf("usage: %s cases.bin out.bin\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { printf("cannot open %s / %s\n", argv[1], argv[2]); return 2; }
    int32_t n[4];
    if (!rd(in, n, 4) || n[0] < 0 || n[1] < 0 || n[2] < 0 || n[3] < 0) { printf("bad header\n"); return 2; }

    std::vector<float> pairs((size_t)n[0] * 6), s32((size_t)n[0]);
    if (!rd(in, pairs.data(), pairs.size())) { printf("short file (pairs)\n"); return 2; }
    for (int i = 0; i < n[0]; ++i) {
        const float* p = &pairs[(size_t)i * 6];
        s32[i] = ch_dist2(p[0], p[1], p[2], p[3], p[4], p[5]);
        CHECK(s32[i] == ch_dist2(p[3], p[4], p[5], p[0], p[1], p[2]));          // (the squares do not see the sign)
    }
    wr(out, s32.data(), s32.size());

    std::vector<double> rin((size_t)n[1] * 4), rout((size_t)n[1] * 4);
    if (!rd(in, rin.data(), rin.size())) { printf("short file (rho)\n"); return 2; }
    for (int i = 0; i < n[1]; ++i) {
        const float s = (float)rin[(size_t)i * 4], rho = (float)rin[(size_t)i * 4 + 1], w = (float)rin[(size_t)i * 4 + 2], g = (float)rin[(size_t)i * 4 + 3];
        const double r2 = ch_rho2(rho);
        rout[(size_t)i * 4] = ch_rho((double)s, r2);
        rout[(size_t)i * 4 + 1] = ch_drho((double)s, r2);
        rout[(size_t)i * 4 + 2] = (double)ch_point_value(s, w, r2);
        rout[(size_t)i * 4 + 3] = ch_coef(g, w, s, r2);
        if (rho == 0.f) { CHECK(rout[(size_t)i * 4] == (double)s); CHECK(rout[(size_t)i * 4 + 1] == 1.0); }
        else CHECK(rout[(size_t)i * 4] <= r2);                                    // (the GMoF saturates at rho^2)
    }
    wr(out, rout.data(), rout.size());

    std::vector<int32_t> lens((size_t)n[2]), segs((size_t)n[2]);
    if (!rd(in, lens.data(), lens.size())) { printf("short file (lengths)\n"); return 2; }
    for (int i = 0; i < n[2]; ++i) {
        segs[i] = ch_seg_len(lens[i]);
        const int n_seg = (lens[i] + segs[i] - 1) / segs[i];
        CHECK(segs[i] >= 1 && n_seg <= CH_SEGMENTS && (lens[i] > CH_SERIAL_MAX || n_seg == 1));
    }
    wr(out, segs.data(), segs.size());

    for (int c = 0; c < n[3]; ++c) {
        int32_t d[2];
        if (!rd(in, d, 2) || d[0] < 0 || d[1] < 1) { printf("short file (index case %d)\n", c); return 2; }
        const int nq = d[0], nt = d[1];
        std::vector<int32_t> idx((size_t)nq), off((size_t)nt + 1), list((size_t)nq, -1);
        if (!rd(in, idx.data(), idx.size())) { printf("short file (indices of case %d)\n", c); return 2; }
        const int total = ch_invert(idx.data(), nq, nt, off.data(), list.data());
        CHECK(off[0] == 0 && off[nt] == total);
        for (int t = 0; t < nt; ++t) {
            CHECK(off[t] <= off[t + 1]);
            for (int k = off[t]; k < off[t + 1]; ++k) {
                CHECK(idx[list[k]] == t);
                if (k > off[t]) CHECK(list[k - 1] < list[k]);
            }
        }
        // the device's way: any fill order, then every entry to its rank
        std::vector<int32_t> cursor((size_t)nt, 0), loose((size_t)nq, -1), placed((size_t)nq, -1);
        for (int step = 0; step < nq; ++step) {
            const int q = (int)(((long long)step * 7919 + 13) % (nq > 0 ? nq : 1));           // 7919 is prime: a permutation unless it divides nq
            if (ch_index_ok(idx[q], nt)) loose[off[idx[q]] + cursor[idx[q]]++] = q;
        }
        CHECK(nq == 0 || nq % 7919 != 0);
        for (int q = 0; q < nq; ++q) {
            if (!ch_index_ok(idx[q], nt)) continue;
            const int o = off[idx[q]], len = off[idx[q] + 1] - o;
            placed[o + ch_rank(&loose[o], len, q)] = q;
        }
        for (int k = 0; k < nq; ++k) CHECK(placed[k] == list[k]);
        wr(out, off.data(), off.size());
        wr(out, list.data(), list.size());
        wr(out, placed.data(), placed.size());
    }
    fclose(in);
    fclose(out);
    printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
