// CPU run of the optimiser's scalar layer (csrc/lbfgs_scalar.h): reads float64 records from the file named first and writes the
// header's answers, float64 too, to the file named second.  Stand-alone: own main, no device.  Built and run by
// tests/test_lbfgs_scalar_host.py (host AddressSanitizer + UBSan), which compares every answer with the specification
// (oracle/lbfgs_machine.py, oracle/fit_frame.py).
//   in:   n_cubic, n_flip, then per cubic case 10 numbers: x1 f1 g1 x2 f2 g2 lo hi (values), the tags of those eight as a bit
//         mask (bit i: value i is a 0-d tensor), has_bounds; per flip case 3 numbers (a float32 rotation vector)
//   out:  per cubic case value and tag; per flip case 3 numbers; then fresh_state(): the fields named in the last loop below
#include "../smplify-x-partial_amd/csrc/lbfgs_scalar.h"
#include <cstdio>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 3) { printf("usage: %s in.bin out.bin\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { printf("cannot read %s\n", argv[1]); return 2; }
    std::vector<double> rec;
    double buf[256];
    for (size_t n; (n = fread(buf, sizeof(double), 256, in)) > 0;) rec.insert(rec.end(), buf, buf + n);
    fclose(in);
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
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(out.data(), sizeof(double), out.size(), o) != out.size()) { printf("cannot write %s\n", argv[2]); return 2; }
    fclose(o);
    printf("%zu cubic steps, %zu flipped orientations, sizeof(OptScal) = %zu\n", n_cubic, n_flip, sizeof(OptScal));
    return 0;
}
