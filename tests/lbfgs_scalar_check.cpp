// CPU run of the optimiser's scalar layer (csrc/lbfgs_scalar.h): reads float64 records from the file named first and writes the
// header's answers, float64 too, to the file named second.  Stand-alone: own main, no device.  Built and run by
// tests/test_lbfgs_scalar_host.py (host AddressSanitizer + UBSan), which compares every answer with the specification
// (oracle/lbfgs_machine.py, oracle/fit_frame.py).
//   in:   n_cubic, n_flip, then per cubic case 10 numbers: x1 f1 g1 x2 f2 g2 lo hi (values), the tags of those eight as a bit
//         mask (bit i: value i is a 0-d tensor), has_bounds; per flip case 3 numbers (a float32 rotation vector)
//   out:  per cubic case value and tag; per flip case 3 numbers; then fresh_state(): the fields named in the last loop below
//
// With two more file names, the line search's transitions (ls_bracket_eval, ls_zoom_eval, ls_zoom_trial) on seeded states:
//   in:   per case TR_IN numbers: kind (0 bracket phase, 1 zoom phase, 2 zoom trial); the 13 scalars of the state named in
//         `sc` below as (value, tag) pairs; ls_iter ls_evals ls_done insuf low high; f_in (a Python float), gtd_new (a
//         tensor); max_ls, max_iter, tol_change
//   out:  per case TR_OUT numbers: what the transition returned (three numbers; unused ones 0), phase, the 13 scalars as (value,
//         tag) pairs, the six integers
#include "../smplify-x-partial_amd/csrc/lbfgs_scalar.h"
#include <cstdio>
#include <vector>

enum { TR_IN = 1 + 26 + 6 + 2 + 3, TR_OUT = 4 + 26 + 6 };

static bool read_doubles(const char* path, std::vector<double>& rec) {
    FILE* in = fopen(path, "rb");
    if (!in) { printf("cannot read %s\n", path); return false; }
    double buf[256];
    for (size_t n; (n = fread(buf, sizeof(double), 256, in)) > 0;) rec.insert(rec.end(), buf, buf + n);
    fclose(in);
    return true;
}
static bool write_doubles(const char* path, const std::vector<double>& out) {
    FILE* o = fopen(path, "wb");
    if (!o || fwrite(out.data(), sizeof(double), out.size(), o) != out.size()) { printf("cannot write %s\n", path); return false; }
    fclose(o);
    return true;
}

static int transitions(const char* in_path, const char* out_path) {
    std::vector<double> rec, out;
    if (!read_doubles(in_path, rec)) return 2;
    if (rec.size() % TR_IN) { printf("%zu numbers are no whole transition cases\n", rec.size()); return 2; }
    size_t n_kind[3] = {0, 0, 0};
    for (const double* r = rec.data(); r < rec.data() + rec.size(); r += TR_IN) {
        OptScal s = fresh_state();
        Sc* const sc[13] = {&s.t, &s.t_prev, &s.f_prev, &s.gtd_prev, &s.ls_f0, &s.ls_gtd0, &s.d_norm, &s.br0, &s.br1, &s.bf0, &s.bf1, &s.bgtd0, &s.bgtd1};
        for (int k = 0; k < 13; ++k) *sc[k] = r[2 + 2 * k] != 0.0 ? T((float)r[1 + 2 * k]) : P(r[1 + 2 * k]);
        const double* q = r + 27;
        s.ls_iter = (int)q[0]; s.ls_evals = (int)q[1]; s.ls_done = (int)q[2]; s.insuf = (int)q[3]; s.low = (int)q[4]; s.high = (int)q[5];
        const Sc f_in = P(q[6]), gtd_new = T((float)q[7]);
        const int kind = (int)r[0], max_ls = (int)q[8], max_iter = (int)q[9];
        const double tol_change = q[10];
        double ret[3] = {0, 0, 0};
        if (kind == 0) { s.phase = PH_BRACKET; ret[0] = ls_bracket_eval(s, f_in, gtd_new, max_ls); }
        else if (kind == 1) { s.phase = PH_ZOOM; const ZoomMove m = ls_zoom_eval(s, f_in, gtd_new, tol_change); ret[0] = m.end; ret[1] = m.copy_first; ret[2] = m.collapsed; }
        else if (kind == 2) { s.phase = PH_BRACKET; ret[0] = ls_zoom_trial(s, max_iter) ? 1 : 0; }
        else { printf("transition kind %d\n", kind); return 2; }
        n_kind[kind] += 1;
        out.insert(out.end(), ret, ret + 3);
        out.push_back((double)s.phase);
        for (int k = 0; k < 13; ++k) { out.push_back(sc[k]->v); out.push_back((double)sc[k]->t); }
        for (int v : {s.ls_iter, s.ls_evals, s.ls_done, s.insuf, s.low, s.high}) out.push_back((double)v);
    }
    if (!write_doubles(out_path, out)) return 2;
    printf("%zu bracket-phase, %zu zoom-phase evaluations, %zu zoom trials\n", n_kind[0], n_kind[1], n_kind[2]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3 && argc != 5) { printf("usage: %s in.bin out.bin [transitions_in.bin transitions_out.bin]\n", argv[0]); return 2; }
    if (argc == 5) { const int rc = transitions(argv[3], argv[4]); if (rc) return rc; }
    std::vector<double> rec;
    if (!read_doubles(argv[1], rec)) return 2;
    if (rec.size() < 2) { printf("no header\n"); return 2; }
    const size_t n_cubic = (size_t)rec[0], n_flip = (size_t)rec[1];
    if (rec.size() != 2 + 10 * n_cubic + 3 * n_flip) { printf("%zu numbers for %zu + %zu cases\n", rec.size(), n_cubic, n_flip); return 2; }
    std::vector<double> out;
    const double* r = &rec[2];
    for (size_t i = 0; i < n_cubic; ++i, r += 10) {
        Sc a[8];
        const int tags = (int)r[8];
        for (int k = 0; k < 8; ++k) a[k] = ((tags >> k) & 1) ? T((float)r[k]) : P(r[k]);
        const Sc t = cubic_interpolate(a[0], a[1], a[2], a[3], a[4], a[5], r[9] != 0.0, a[6], a[7]);
        out.push_back(t.v); out.push_back((double)t.t);
    }
    for (size_t i = 0; i < n_flip; ++i, r += 3) {
        const float go[3] = {(float)r[0], (float)r[1], (float)r[2]};
        float fl[3];
        flipped_orientation(go, fl);
        for (float v : fl) out.push_back((double)v);
    }
    const OptScal s = fresh_state();
    for (double v : {(double)s.phase, (double)s.outer, (double)s.n_iter_total, (double)s.func_evals, (double)s.evals, s.H_diag.v,
                     (double)s.H_diag.t, (double)s.hist_n, (double)s.cache_valid, (double)s.has_prev_outer})
        out.push_back(v);
    if (!write_doubles(argv[2], out)) return 2;
    printf("%zu cubic steps, %zu flipped orientations, sizeof(OptScal) = %zu\n", n_cubic, n_flip, sizeof(OptScal));
    return 0;
}
