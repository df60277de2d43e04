// Stand-alone host build of the 1-4 plane per-pixel functions (include/yolomi_augment.h).
//   augment_colour_host render <cases.bin> <out.bin> <ch> [colour.bin]
//       reads a case file (tests/augment_ref.py write_case_file; the images pixel-interleaved, h0 * w0 * ch bytes
//       each) and, optionally, one ym_aug_colour per table entry; evaluates every entry over S x S pixels with
//       ym_aug_sample_c and writes the bytes planar, (entry, ch, S, S)
//   augment_colour_host hsv <hue> <sat> <out.bin>
//       ym_aug_hue_sat over all 2^24 colours in the order (r << 16) | (g << 8) | b, three bytes each
// The source buffer is allocated at its exact size, so a build with -fsanitize=address,undefined reports any tap
// outside it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "yolomi_augment.h"

static_assert(sizeof(ym_aug_colour) == 8, "ym_aug_colour layout (yolomi/_lib.py)");

static bool read_all(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

static bool write_file(const char* path, const std::vector<uint8_t>& out) {
    FILE* g = fopen(path, "wb");
    if (!g) return false;
    const bool ok = fwrite(out.data(), 1, out.size(), g) == out.size();
    return fclose(g) == 0 && ok;
}

static int render(int argc, char** argv) {
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    const int ch = atoi(argv[4]);
    int64_t hdr[4];
    if (ch < 1 || ch > 4 || !read_all(f, hdr, sizeof hdr)) return 2;
    const int64_t B = hdr[0], S = hdr[1], n = hdr[2], nbytes = hdr[3];
    if (B < 0 || S <= 0 || S > 32768 || n < 0 || nbytes < 0) return 2;
    std::vector<int64_t> meta(size_t(3 * B));
    uint8_t* src = static_cast<uint8_t*>(malloc(size_t(nbytes ? nbytes : 1)));
    std::vector<ym_aug_entry> table(static_cast<size_t>(n));
    if (!src || !read_all(f, meta.data(), meta.size() * sizeof(int64_t)) || !read_all(f, src, size_t(nbytes)) ||
        !read_all(f, table.data(), table.size() * sizeof(ym_aug_entry)))
        return 2;
    fclose(f);
    std::vector<ym_aug_colour> colour;
    if (argc == 6) {
        if (ch != 3) return 2;                             // as ym_augment_u8c: a colour table needs three planes
        FILE* c = fopen(argv[5], "rb");
        colour.resize(size_t(n));
        if (!c || !read_all(c, colour.data(), colour.size() * sizeof(ym_aug_colour))) return 2;
        fclose(c);
    }
    std::vector<uint8_t> out(size_t(n * ch * S * S));
    for (int64_t i = 0; i < n; ++i)
        for (int y = 0; y < S; ++y)
            for (int x = 0; x < S; ++x) {
                int v[4];
                ym_aug_sample_c(src, meta.data(), int(B), ch, int(S), &table[size_t(i)],
                                colour.empty() ? nullptr : &colour[size_t(i)], x, y, v);
                for (int c = 0; c < ch; ++c) out[size_t(((i * ch + c) * S + y) * S + x)] = uint8_t(v[c]);
            }
    free(src);
    return write_file(argv[3], out) ? 0 : 2;
}

static int hsv(char** argv) {
    const int hue = atoi(argv[2]), sat = atoi(argv[3]);
    std::vector<uint8_t> out(size_t(3) << 24);
    for (int i = 0; i < (1 << 24); ++i) {
        int v[3] = {i >> 16, (i >> 8) & 255, i & 255};
        ym_aug_hue_sat(hue, sat, v);
        for (int c = 0; c < 3; ++c) {
            if (v[c] < 0 || v[c] > 255) return 3;          // outside a byte: reported, not wrapped
            out[size_t(i) * 3 + c] = uint8_t(v[c]);
        }
    }
    return write_file(argv[4], out) ? 0 : 2;
}

int main(int argc, char** argv) {
    if ((argc == 5 || argc == 6) && !strcmp(argv[1], "render")) return render(argc, argv);
    if (argc == 5 && !strcmp(argv[1], "hsv")) return hsv(argv);
    fprintf(stderr, "usage: %s render cases.bin out.bin ch [colour.bin] | hsv hue sat out.bin\n", argv[0]);
    return 2;
}
