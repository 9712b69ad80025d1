// CPU check of the 3x3 Procrustes solve (csrc/procrustes3.h): reads float64 K matrices (row-major, 9 doubles each) from the file
// named first, writes R (9 doubles) and the singular values (3) of each to the file named second, and checks for every K what
// defines the answer:  R^T R = I to 1e-14,  det R = +1,  R K symmetric to 1e-12 |K|,  tr(R K) >= tr(Q K) for 1 000 random
// rotations Q.  Stand-alone: own main, no device.  Built and run by tests/test_procrustes3_host.py (host AddressSanitizer + UBSan),
// which compares the R written here with numpy's V Z U^T.
#include "../smplify-x-partial_amd/csrc/procrustes3.h"
#include <cstdint>
#include <cstdio>
#include <vector>

static int g_fail = 0, g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { if (++g_fail <= 40) printf("FAIL %s:%d  matrix %d  %s\n", __FILE__, __LINE__, g_matrix, #c); } } while (0)
static int g_matrix = -1;

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static double uniform() {        // (-1, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(g_state >> 11) + 0.5) / 4503599627370496.0 - 1.0;
}
static void random_rotation(double* Q) {       // a random unit quaternion as a matrix
    double q[4], n;
    do {
        for (double& x : q) x = uniform();
        n = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    } while (n > 1.0 || n < 1e-3);
    n = sqrt(n);
    const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
    const double M[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    for (int i = 0; i < 9; ++i) Q[i] = M[i];
}
static double trace_of_product(const double* A, const double* B) {
    double t = 0.0;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) t += A[r * 3 + c] * B[c * 3 + r];
    return t;
}

int main(int argc, char** argv) {
    if (argc != 3) { printf("usage: %s K.bin R.bin\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { printf("cannot read %s\n", argv[1]); return 2; }
    std::vector<double> Ks;
    double buf[9];
    while (fread(buf, sizeof(double), 9, in) == 9) Ks.insert(Ks.end(), buf, buf + 9);
    fclose(in);
    const int n = (int)(Ks.size() / 9);
    std::vector<double> out((size_t)n * 12);
    for (g_matrix = 0; g_matrix < n; ++g_matrix) {
        const double* K = &Ks[(size_t)g_matrix * 9];
        double* R = &out[(size_t)g_matrix * 12];
        double* sv = R + 9;
        procrustes3_rotation(K, R, sv);
        double kn = 0.0;
        for (int i = 0; i < 9; ++i) kn += K[i] * K[i];
        kn = sqrt(kn);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                double d = 0.0;
                for (int k = 0; k < 3; ++k) d += R[k * 3 + r] * R[k * 3 + c];
                CHECK(fabs(d - (r == c ? 1.0 : 0.0)) <= 1e-14);
            }
        const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
        CHECK(fabs(det - 1.0) <= 1e-13);
        double RK[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) RK[r * 3 + c] = R[r * 3] * K[c] + R[r * 3 + 1] * K[3 + c] + R[r * 3 + 2] * K[6 + c];
        CHECK(fabs(RK[1] - RK[3]) <= 1e-12 * kn && fabs(RK[2] - RK[6]) <= 1e-12 * kn && fabs(RK[5] - RK[7]) <= 1e-12 * kn);
        const double best = trace_of_product(R, K);
        CHECK(sv[0] >= sv[1] && sv[1] >= sv[2] && sv[2] >= 0.0);
        // tr(R K) = s1 + s2 +- s3: the largest value any rotation reaches
        CHECK(fabs(best - (sv[0] + sv[1] + sv[2])) <= 1e-12 * kn || fabs(best - (sv[0] + sv[1] - sv[2])) <= 1e-12 * kn);
        for (int q = 0; q < 1000; ++q) {
            double Q[9];
            random_rotation(Q);
            CHECK(best >= trace_of_product(Q, K) - 1e-14 * kn);
        }
    }
    // degenerate input stays finite and proper: the zero matrix and a rank-1 matrix
    {
        g_matrix = -2;
        const double Z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, one[9] = {2, 4, 6, 1, 2, 3, -1, -2, -3};
        double R[9], sv[3];
        procrustes3_rotation(Z, R, sv);
        for (int i = 0; i < 9; ++i) CHECK(R[i] == (i % 4 == 0 ? 1.0 : 0.0));
        procrustes3_rotation(one, R, sv);
        const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
        CHECK(fabs(det - 1.0) <= 1e-13 && sv[1] <= 1e-14 * sv[0]);
        CHECK(fabs(trace_of_product(R, one) - sv[0]) <= 1e-12 * sv[0]);
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(out.data(), sizeof(double), out.size(), o) != out.size()) { printf("cannot write %s\n", argv[2]); return 2; }
    fclose(o);
    printf("%d matrices\n%d checks, %d failed\n", n, g_checks, g_fail);
    return g_fail ? 1 : 0;
}
