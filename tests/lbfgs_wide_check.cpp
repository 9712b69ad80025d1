// Stand-alone CPU program for tests/test_opt_wide_host.py: runs the state machine of csrc/lbfgs_wide.h over a serial vector layer
// on recorded evaluations and writes the trial points it asked for, its trace records and its result.
//
//   lbfgs_wide_check in_hdr.bin in_vec.bin out_hdr.bin out_vec.bin
// in_hdr  (float64): n_cases, then per case N, n_evals, maxiters, ftol, gtol, lr, max_iter, max_eval, history, tol_grad, tol_change,
//                    reuse, n_groups, the group lengths, and the n_evals losses
// in_vec  (float32): per case x0 [N], then the n_evals gradients [N]
// out_hdr (float64): per case consumed evaluations, status, result, evals counter, n_records, the records [4] each
// out_vec (float32): per case the trial point before every consumed evaluation [N], then the accepted point [N]
// Built for the host only, with AddressSanitizer and UBSan.
#include "../smplify-x-partial_amd/csrc/lbfgs_wide.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

struct Serial {
    typedef float* Row;
    typedef std::vector<float> Reg;
    int N, slots;
    std::vector<float> rows, hist, al_, ro_;
    std::vector<double> records;
    OptScal scal_;
    OptScal& scal() { return scal_; }
    Serial(int n, int hist_cap) : N(n), slots(wide_ring_slots(hist_cap)), rows((size_t)W_NROWS * n, 0.f),
                                  hist((size_t)2 * wide_ring_slots(hist_cap) * n, 0.f), al_(SFX_HIST_MAX, 0.f), ro_(SFX_HIST_MAX + 1, 0.f) {}
    Row row(int k) { return rows.data() + (size_t)k * N; }
    Row hist_y(int slot) { return hist.data() + (size_t)slot * N; }
    Row hist_s(int slot) { return hist.data() + (size_t)(slots + slot) * N; }
    float* al() { return al_.data(); }
    float* ro() { return ro_.data(); }
    bool leader() const { return true; }
    void sync() {}
    void trace(int ty, double a, double b, double c) { records.push_back(ty); records.push_back((float)a); records.push_back((float)b); records.push_back((float)c); }
    void dots(int n, const Row* a, const Row* b, float* out) {
        for (int k = 0; k < n; ++k) {
            double acc = 0.0;
            for (int i = 0; i < N; ++i) acc += (double)a[k][i] * (double)b[k][i];
            out[k] = (float)acc;
        }
    }
    float dot(Row a, Row b) { float r; dots(1, &a, &b, &r); return r; }
    void axpy(Row dst, Row x, float a, Row y) { for (int i = 0; i < N; ++i) dst[i] = fmaf(a, y[i], x[i]); }
    void copy(Row dst, Row src) { for (int i = 0; i < N; ++i) dst[i] = src[i]; }
    void neg(Row dst, Row src) { for (int i = 0; i < N; ++i) dst[i] = -src[i]; }
    void sub(Row dst, Row a, Row b) { for (int i = 0; i < N; ++i) dst[i] = a[i] - b[i]; }
    void scale(Row dst, Row a, float f) { for (int i = 0; i < N; ++i) dst[i] = a[i] * f; }
    float asum(Row a) { double acc = 0.0; for (int i = 0; i < N; ++i) acc += fabs((double)a[i]); return (float)acc; }
    float amax(Row a) { float m = 0.f; for (int i = 0; i < N; ++i) m = fmaxf(m, fabsf(a[i])); return m; }
    float amax_scaled(Row a, float f) { float m = 0.f; for (int i = 0; i < N; ++i) m = fmaxf(m, fabsf(a[i] * f)); return m; }
    float gmax(Row a, int off, int len) { float m = -INFINITY; for (int i = off; i < off + len; ++i) m = fmaxf(m, a[i]); return m; }
    void r_load_neg(Reg& q, Row a) { q.resize(N); for (int i = 0; i < N; ++i) q[i] = -a[i]; }
    float r_dot(Reg& q, Row a) { double acc = 0.0; for (int i = 0; i < N; ++i) acc += (double)q[i] * (double)a[i]; return (float)acc; }
    void r_axpy(Reg& q, float a, Row y) { for (int i = 0; i < N; ++i) q[i] = fmaf(a, y[i], q[i]); }
    void r_scale(Reg& q, float f) { for (int i = 0; i < N; ++i) q[i] = q[i] * f; }
    void r_store(Row dst, Reg& q) { for (int i = 0; i < N; ++i) dst[i] = q[i]; }
};

template <typename T> static std::vector<T> slurp(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)n / sizeof(T));
    if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "short read of %s\n", path); exit(2); }
    fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc != 5) { fprintf(stderr, "usage: %s in_hdr in_vec out_hdr out_vec\n", argv[0]); return 2; }
    const std::vector<double> hdr = slurp<double>(argv[1]);
    const std::vector<float> vec = slurp<float>(argv[2]);
    std::vector<double> ohdr;
    std::vector<float> ovec;
    size_t h = 0, p = 0;
    const int n_cases = (int)hdr.at(h++);
    for (int c = 0; c < n_cases; ++c) {
        WideCfg C{};
        C.N = (int)hdr.at(h++);
        const int n_evals = (int)hdr.at(h++);
        C.maxiters = (int)hdr.at(h++); C.ftol = hdr.at(h++); C.gtol = hdr.at(h++); C.lr = (float)hdr.at(h++);
        C.max_iter = (int)hdr.at(h++); C.max_eval = (int)hdr.at(h++); C.hist_cap = (int)hdr.at(h++);
        C.tol_grad = hdr.at(h++); C.tol_change = hdr.at(h++); C.reuse = (int)hdr.at(h++);
        C.ngroups = (int)hdr.at(h++);
        std::vector<int> g_off(C.ngroups), g_len(C.ngroups);
        for (int i = 0, o = 0; i < C.ngroups; ++i) { g_len[i] = (int)hdr.at(h++); g_off[i] = o; o += g_len[i]; }
        C.g_off = g_off.data(); C.g_len = g_len.data();
        if (C.N < 1 || C.N > SFX_WIDE_NMAX || C.hist_cap < 1 || C.hist_cap > SFX_HIST_MAX || h + n_evals > hdr.size() ||
            p + (size_t)(1 + n_evals) * C.N > vec.size()) { fprintf(stderr, "case %d: bad header\n", c); return 2; }
        const double* losses = &hdr[h]; h += n_evals;
        Serial v(C.N, C.hist_cap);
        WideState st{};
        for (int i = 0; i < C.N; ++i) v.row(W_X)[i] = vec[p + i];
        p += C.N;
        wide_begin(v, st, 1);
        int k = 0;
        for (; k < n_evals && st.status == WIDE_RUNNING; ++k) {
            ovec.insert(ovec.end(), v.row(W_XT), v.row(W_XT) + C.N);
            for (int i = 0; i < C.N; ++i) v.row(W_GIN)[i] = vec[p + (size_t)k * C.N + i];
            wide_tick(v, C, st, 0, (float)losses[k]);
        }
        p += (size_t)n_evals * C.N;
        ovec.insert(ovec.end(), v.row(W_X), v.row(W_X) + C.N);
        ohdr.push_back(k); ohdr.push_back(st.status); ohdr.push_back(st.result); ohdr.push_back(st.evals);
        ohdr.push_back((double)(v.records.size() / 4));
        ohdr.insert(ohdr.end(), v.records.begin(), v.records.end());
    }
    FILE* f = fopen(argv[3], "wb");
    if (!f || fwrite(ohdr.data(), sizeof(double), ohdr.size(), f) != ohdr.size()) return 2;
    fclose(f);
    f = fopen(argv[4], "wb");
    if (!f || fwrite(ovec.data(), sizeof(float), ovec.size(), f) != ovec.size()) return 2;
    fclose(f);
    printf("%d cases, sizeof(WideState) = %d\n", n_cases, (int)sizeof(WideState));
    return 0;
}
