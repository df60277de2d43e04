// Stand-alone host build of ym_tile_sample_c (include/yolomi_augment.h) for the mirrored views of test-time
// augmentation.
//   tta_host <cases.bin> <out.bin>
//       reads a case file (tests/slice_ref.py write_case_file) and evaluates every tile over H x W pixels four times,
//       with the mirror bits of its `edges` replaced by 0, YM_TILE_MIRROR_X, YM_TILE_MIRROR_Y and both; writes the
//       bytes planar, (bits, tile, ch, H, W)
// The source buffer is allocated at its exact size: under -fsanitize=address,undefined a reflected index that left the
// window would be reported.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "yolomi_augment.h"

static bool read_all(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t hdr[7];
    if (!read_all(f, hdr, sizeof hdr)) return 2;
    const int64_t B = hdr[0], T = hdr[1], H = hdr[2], W = hdr[3], ch = hdr[4], fill = hdr[5], nbytes = hdr[6];
    if (B < 0 || B > 65535 || T < 0 || T > 65535 || H <= 0 || H > 32768 || W <= 0 || W > 32768 || ch < 1 || ch > 4 ||
        nbytes < 0)
        return 2;
    std::vector<int64_t> meta(size_t(3 * B));
    uint8_t* src = static_cast<uint8_t*>(malloc(size_t(nbytes ? nbytes : 1)));
    std::vector<ym_tile_entry> table(static_cast<size_t>(T));
    if (!src || !read_all(f, meta.data(), meta.size() * sizeof(int64_t)) || !read_all(f, src, size_t(nbytes)) ||
        !read_all(f, table.data(), table.size() * sizeof(ym_tile_entry)))
        return 2;
    fclose(f);
    static const int BITS[4] = {0, YM_TILE_MIRROR_X, YM_TILE_MIRROR_Y, YM_TILE_MIRROR_X | YM_TILE_MIRROR_Y};
    std::vector<uint8_t> out(size_t(4 * T * ch * H * W));
    size_t o = 0;
    for (int m = 0; m < 4; ++m)
        for (int64_t t = 0; t < T; ++t) {
            ym_tile_entry e = table[size_t(t)];
            e.edges = (e.edges & ~(YM_TILE_MIRROR_X | YM_TILE_MIRROR_Y)) | BITS[m];
            for (int c = 0; c < ch; ++c)
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x) {
                        int v[4];
                        ym_tile_sample_c(src, meta.data(), int(B), int(ch), &e, int(fill), x, y, v);
                        if (v[c] < 0 || v[c] > 255) return 3;      // outside a byte: reported, not wrapped
                        out[o++] = uint8_t(v[c]);
                    }
        }
    free(src);
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    const bool ok = fwrite(out.data(), 1, out.size(), g) == out.size();
    return fclose(g) == 0 && ok ? 0 : 2;
}
