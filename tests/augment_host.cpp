// Stand-alone host build of the augmentation's per-pixel function (include/yolomi_augment.h): reads a case file
// (tests/augment_ref.py write_case_file), evaluates every table entry over S x S pixels with ym_aug_sample and
// writes the bytes.  The source buffer is allocated at its exact size, so a build with -fsanitize=address,undefined
// reports any tap outside it.
//   augment_host <cases.bin> <out.bin>
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
    int64_t hdr[4];
    if (!read_all(f, hdr, sizeof hdr)) return 2;
    const int64_t B = hdr[0], S = hdr[1], n = hdr[2], nbytes = hdr[3];
    if (B < 0 || S <= 0 || S > 32768 || n < 0 || nbytes < 0) return 2;
    std::vector<int64_t> meta(size_t(3 * B));
    uint8_t* src = static_cast<uint8_t*>(malloc(size_t(nbytes ? nbytes : 1)));
    std::vector<ym_aug_entry> table(static_cast<size_t>(n));
    if (!src || !read_all(f, meta.data(), meta.size() * sizeof(int64_t)) || !read_all(f, src, size_t(nbytes)) ||
        !read_all(f, table.data(), table.size() * sizeof(ym_aug_entry)))
        return 2;
    fclose(f);
    std::vector<uint8_t> out(size_t(n * S * S));
    for (int64_t i = 0; i < n; ++i)
        for (int y = 0; y < S; ++y)
            for (int x = 0; x < S; ++x)
                out[size_t((i * S + y) * S + x)] =
                    uint8_t(ym_aug_sample(src, meta.data(), int(B), int(S), &table[size_t(i)], x, y));
    FILE* g = fopen(argv[2], "wb");
    if (!g || fwrite(out.data(), 1, out.size(), g) != out.size()) return 2;
    fclose(g);
    free(src);
    return 0;
}
