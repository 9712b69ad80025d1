// CPU check of the rasteriser's integer coverage arithmetic (csrc/raster_fixed.h: snap, orientation, edge functions, top-left
// rule, clipped pixel box).  Reads triangles from the file named first -- records of  int32 W, H;  float32 x0, y0, x1, y1, x2, y2
// (screen positions in pixels);  float32 z, znear (one depth for the three corners) -- and writes to the file named second, per
// record:  int32 usable (all three corners);  int32 sx[3], sy[3];  int64 area2;  int32 box x0, y0, x1, y1;  then H * W bytes,
// 1 where the pixel centre is covered.  The walk is the device's: the clipped box only.  Checked here for every record: the three
// edge values add up to area2 at every pixel of the box, the box lies inside the image, and an unusable or zero-area triangle
// covers nothing.  Stand-alone: own main, no device.  Built and run by tests/test_raster_fixed_host.py (host AddressSanitizer +
// UBSan), which compares every byte with the numpy oracle's brute-force coverage of the whole image.
#include "../smplify-x-partial_amd/csrc/raster_fixed.h"
#include <cstdio>
#include <cstring>
#include <vector>

static int g_fail = 0, g_checks = 0, g_record = -1;
#define CHECK(c) do { ++g_checks; if (!(c)) { if (++g_fail <= 40) printf("FAIL %s:%d  record %d  %s\n", __FILE__, __LINE__, g_record, #c); } } while (0)

struct Record { int32_t W, H; float xy[6]; float z, znear; };

int main(int argc, char** argv) {
    if (argc != 3) { printf("usage: %s triangles.bin coverage.bin\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { printf("cannot open the files\n"); return 2; }
    Record r;
    while (fread(&r, sizeof r, 1, in) == 1) {
        ++g_record;
        CHECK(r.W >= 1 && r.H >= 1 && (long long)r.W * r.H <= (1 << 24));
        if (r.W < 1 || r.H < 1 || (long long)r.W * r.H > (1 << 24)) break;
        std::vector<unsigned char> mask((size_t)r.W * r.H, 0);
        int32_t usable = 1, x[3] = {0, 0, 0}, y[3] = {0, 0, 0}, box[4] = {0, 0, -1, -1};
        rs_i64 area2 = 0;
        for (int i = 0; i < 3; ++i) usable = usable && rs_usable(r.xy[2 * i], r.xy[2 * i + 1], r.z, r.znear);
        if (usable) {
            for (int i = 0; i < 3; ++i) { x[i] = rs_snap(r.xy[2 * i]); y[i] = rs_snap(r.xy[2 * i + 1]); }
            for (int i = 0; i < 3; ++i) CHECK(x[i] >= -(1 << 28) && x[i] <= (1 << 28) && y[i] >= -(1 << 28) && y[i] <= (1 << 28));
            const RsTri t = rs_setup(x, y);
            area2 = t.area2;
            CHECK(area2 >= 0);
            const RsBox b = rs_box(x, y, r.W, r.H);
            box[0] = b.x0; box[1] = b.y0; box[2] = b.x1; box[3] = b.y1;
            CHECK(b.x0 >= 0 && b.y0 >= 0 && b.x1 <= r.W - 1 && b.y1 <= r.H - 1);
            CHECK(rs_box_pixels(b) >= 0 && rs_box_pixels(b) <= (rs_i64)r.W * r.H);
            if (area2 > 0) {
                for (int32_t py = b.y0; py <= b.y1; ++py)
                    for (int32_t px = b.x0; px <= b.x1; ++px) {
                        rs_i64 e[3];
                        const bool in_tri = rs_covers(t, px, py, e);
                        CHECK(e[0] + e[1] + e[2] == area2);
                        CHECK(in_tri == ((e[0] > 0 || (e[0] == 0 && rs_top_left(t, 0))) && (e[1] > 0 || (e[1] == 0 && rs_top_left(t, 1))) &&
                                         (e[2] > 0 || (e[2] == 0 && rs_top_left(t, 2)))));
                        if (in_tri) mask[(size_t)py * r.W + px] = 1;
                    }
            }
        }
        fwrite(&usable, 4, 1, out); fwrite(x, 4, 3, out); fwrite(y, 4, 3, out); fwrite(&area2, 8, 1, out); fwrite(box, 4, 4, out);
        fwrite(mask.data(), 1, mask.size(), out);
    }
    fclose(in); fclose(out);
    printf("%d records\n%d checks, %d failed\n", g_record + 1, g_checks, g_fail);
    return g_fail ? 1 : 0;
}
