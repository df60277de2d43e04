// Stand-alone host build of ym_letterbox_u8c's per-pixel function (include/yolomi_augment.h: ym_lb_sample_c).
//   letterbox_host <cases.bin> <out.bin>
//       reads a case file (tests/letterbox_ref.py write_case_file: header {B, H, W, ch, fill, n_bytes}, meta, the
//       pixel-interleaved source bytes, one ym_lb_entry per image), evaluates every image over H x W pixels and
//       writes the bytes planar, (image, ch, H, W)
// The source buffer is allocated at its exact size, so a build with -fsanitize=address,undefined reports any tap
// outside it.
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
    int64_t hdr[6];
    if (!read_all(f, hdr, sizeof hdr)) return 2;
    const int64_t B = hdr[0], H = hdr[1], W = hdr[2], ch = hdr[3], fill = hdr[4], nbytes = hdr[5];
    if (B < 0 || H <= 0 || H > 32768 || W <= 0 || W > 32768 || ch < 1 || ch > 4 || nbytes < 0) return 2;
    std::vector<int64_t> meta(size_t(3 * B));
    uint8_t* src = static_cast<uint8_t*>(malloc(size_t(nbytes ? nbytes : 1)));
    std::vector<ym_lb_entry> table(static_cast<size_t>(B));
    if (!src || !read_all(f, meta.data(), meta.size() * sizeof(int64_t)) || !read_all(f, src, size_t(nbytes)) ||
        !read_all(f, table.data(), table.size() * sizeof(ym_lb_entry)))
        return 2;
    fclose(f);
    std::vector<uint8_t> out(size_t(B * ch * H * W));
    for (int64_t b = 0; b < B; ++b)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                int v[4];
                ym_lb_sample_c(src, meta.data(), int(b), int(ch), &table[size_t(b)], int(fill), x, y, v);
                for (int c = 0; c < ch; ++c) {
                    if (v[c] < 0 || v[c] > 255) return 3;      // outside a byte: reported, not wrapped
                    out[size_t(((b * ch + c) * H + y) * W + x)] = uint8_t(v[c]);
                }
            }
    free(src);
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    const bool ok = fwrite(out.data(), 1, out.size(), g) == out.size();
    return fclose(g) == 0 && ok ? 0 : 2;
}
