// CPU check of the point-to-triangle term's arithmetic and bookkeeping (csrc/p2m_math.h over csrc/chamfer_math.h): reads the
// cases tests/test_p2m_host.py wrote to the file named first and writes what the header makes of them to the file named second.
//   in :  int32 n_tri, n_idx
//         n_tri x 12 float32        (p a b c)           -> n_tri x 7 float32 (s u v w qx qy qz) by p2m_closest,
//                                                          n_tri x 12 float64: the point's row c (p - q) and the three corner
//                                                          terms -(c bary_k)(p - q), with c = ch_coef(1, 1, s, 0)
//         n_idx x { int32 np, nv; 3 np x int32 corner } -> int32 off[nv + 1], list[3 np] (padded with -1) by ch_invert,
//                                                          list[3 np] again by the device's way
// Checked here: p2m_closest_staged on differences formed beforehand gives the bits of p2m_closest; u + v + w and the closest
// point stay inside the triangle's bounds where s is a number; the inverted index of the 3 np corner entries e = 3 i + k is an
// exclusive scan with ascending lists both ways (the device's way: a scrambled fill, then every entry to its ch_rank).
// Stand-alone: own main, no device.  Built and run with host AddressSanitizer + UBSan.
#include "../smplify-x-partial_amd/csrc/p2m_math.h"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static int g_fail = 0, g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { if (++g_fail <= 40) printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); } } while (0)

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
static void wr(FILE* f, const T* p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }

static bool same_bits(float x, float y) { return memcmp(&x, &y, sizeof x) == 0 || (x != x && y != y); }

int main(int argc, char** argv) {
    if (argc != 3) { printf("usage: %s cases.bin out.bin\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { printf("cannot open %s / %s\n", argv[1], argv[2]); return 2; }
    int32_t n[2];
    if (!rd(in, n, 2) || n[0] < 0 || n[1] < 0) { printf("bad header\n"); return 2; }

    std::vector<float> tri((size_t)n[0] * 12), hit((size_t)n[0] * 7);
    std::vector<double> rows((size_t)n[0] * 12);
    if (!rd(in, tri.data(), tri.size())) { printf("short file (triangles)\n"); return 2; }
    for (int i = 0; i < n[0]; ++i) {
        const float* p = &tri[(size_t)i * 12]; const float* a = p + 3; const float* b = p + 6; const float* c = p + 9;
        const P2mHit h = p2m_closest(p, a, b, c);
        const float ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
        const P2mHit g = p2m_closest_staged(p, a, b, c, ab, ac);
        CHECK(same_bits(h.s, g.s) && same_bits(h.u, g.u) && same_bits(h.v, g.v) && same_bits(h.w, g.w));
        if (h.s == h.s) {
            CHECK(h.s >= 0.f);
            CHECK(h.v >= -1e-3f && h.w >= -1e-3f && h.u >= -1e-3f && h.v <= 1.001f && h.w <= 1.001f && h.u <= 1.001f);
        }
        float* o = &hit[(size_t)i * 7];
        o[0] = h.s; o[1] = h.u; o[2] = h.v; o[3] = h.w; o[4] = h.q[0]; o[5] = h.q[1]; o[6] = h.q[2];
        const double coef = ch_coef(1.f, 1.f, h.s, 0.0);
        double* r = &rows[(size_t)i * 12];
        double own[3];
        p2m_point_term(p, h, coef, own);
        r[0] = own[0]; r[1] = own[1]; r[2] = own[2];
        for (int k = 0; k < 3; ++k) {
            double acc[3] = {0.0, 0.0, 0.0};
            p2m_corner_term(p, h, k, coef, acc);
            r[3 + 3 * k] = acc[0]; r[4 + 3 * k] = acc[1]; r[5 + 3 * k] = acc[2];
        }
    }
    wr(out, hit.data(), hit.size());
    wr(out, rows.data(), rows.size());

    for (int c = 0; c < n[1]; ++c) {
        int32_t d[2];
        if (!rd(in, d, 2) || d[0] < 0 || d[1] < 1) { printf("short file (index case %d)\n", c); return 2; }
        const int nq = 3 * d[0], nt = d[1];
        std::vector<int32_t> idx((size_t)nq), off((size_t)nt + 1), list((size_t)nq, -1);
        if (!rd(in, idx.data(), idx.size())) { printf("short file (corners of case %d)\n", c); return 2; }
        for (int i = 0; i < d[0]; ++i) for (int k = 0; k < 3; ++k) CHECK(p2m_entry(i, k) == 3 * i + k);
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
