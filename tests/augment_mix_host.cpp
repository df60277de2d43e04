// Stand-alone host build of the MixUp per-pixel functions (include/yolomi_augment.h).
//   augment_mix_host render <cases.bin> <mix.bin> <out.bin> <ch> [colour.bin]
//       reads a case file (tests/augment_ref.py write_case_file; the images pixel-interleaved, h0 * w0 * ch bytes
//       each) holding one primary ym_aug_entry per image, a mix file (tests/augment_mix_ref.py write_mix_file: int64
//       {n_partner, n_mix}, the partner entries, one ym_aug_mix per image) and, optionally, one ym_aug_colour per
//       image; evaluates every image over S x S pixels with ym_aug_mix_sample_c and writes the bytes planar,
//       (image, ch, S, S)
//   augment_mix_host blend <ratio> <out.bin>
//       ym_aug_mix_blend at ym_aug_mix_ratio(ratio) over all 65536 (a, p) pairs in the order (a << 8) | p, one byte each
// The source buffer and both tables are allocated at their exact sizes (no partner table at all when n_partner is 0),
// so a build with -fsanitize=address,undefined reports any tap or table read outside them.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "yolomi_augment.h"

static bool read_all(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

static bool write_file(const char* path, const std::vector<uint8_t>& out) {
    FILE* g = fopen(path, "wb");
    if (!g) return false;
    const bool ok = fwrite(out.data(), 1, out.size(), g) == out.size();
    return fclose(g) == 0 && ok;
}

template <class T>
static T* exact(size_t n) { return n ? static_cast<T*>(malloc(n * sizeof(T))) : nullptr; }

static int render(int argc, char** argv) {
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    const int ch = atoi(argv[5]);
    int64_t hdr[4];
    if (ch < 1 || ch > 4 || !read_all(f, hdr, sizeof hdr)) return 2;
    const int64_t B = hdr[0], S = hdr[1], n = hdr[2], nbytes = hdr[3];
    if (B < 0 || S <= 0 || S > 32768 || n < 0 || nbytes < 0) return 2;
    std::vector<int64_t> meta(size_t(3 * B));
    uint8_t* src = static_cast<uint8_t*>(malloc(size_t(nbytes ? nbytes : 1)));
    ym_aug_entry* table = exact<ym_aug_entry>(size_t(n));
    if (!src || (n && !table) || !read_all(f, meta.data(), meta.size() * sizeof(int64_t)) ||
        !read_all(f, src, size_t(nbytes)) || !read_all(f, table, size_t(n) * sizeof(ym_aug_entry)))
        return 2;
    fclose(f);

    FILE* m = fopen(argv[3], "rb");
    int64_t mh[2];
    if (!m || !read_all(m, mh, sizeof mh) || mh[0] < 0 || mh[0] > INT32_MAX || mh[1] != n) return 2;
    const int n_partner = int(mh[0]);
    ym_aug_entry* partner = exact<ym_aug_entry>(size_t(n_partner));
    ym_aug_mix* mix = exact<ym_aug_mix>(size_t(n));
    if ((n_partner && !partner) || (n && !mix) || !read_all(m, partner, size_t(n_partner) * sizeof(ym_aug_entry)) ||
        !read_all(m, mix, size_t(n) * sizeof(ym_aug_mix)))
        return 2;
    fclose(m);

    ym_aug_colour* colour = nullptr;
    if (argc == 7) {
        if (ch != 3) return 2;                             // as ym_augment_mix_u8c: a colour table needs three planes
        FILE* c = fopen(argv[6], "rb");
        colour = exact<ym_aug_colour>(size_t(n));
        if (!c || (n && !colour) || !read_all(c, colour, size_t(n) * sizeof(ym_aug_colour))) return 2;
        fclose(c);
    }
    std::vector<uint8_t> out(size_t(n * ch * S * S));
    for (int64_t i = 0; i < n; ++i)
        for (int y = 0; y < S; ++y)
            for (int x = 0; x < S; ++x) {
                int v[4];
                ym_aug_mix_sample_c(src, meta.data(), int(B), ch, int(S), table + i, mix + i, partner, n_partner,
                                    colour ? colour + i : nullptr, x, y, v);
                for (int c = 0; c < ch; ++c) {
                    if (v[c] < 0 || v[c] > 255) return 3;  // outside a byte: reported, not wrapped
                    out[size_t(((i * ch + c) * S + y) * S + x)] = uint8_t(v[c]);
                }
            }
    free(src), free(table), free(partner), free(mix), free(colour);
    return write_file(argv[4], out) ? 0 : 2;
}

static int blend(char** argv) {
    const int r = ym_aug_mix_ratio(atoi(argv[2]));
    std::vector<uint8_t> out(size_t(1) << 16);
    for (int a = 0; a < 256; ++a)
        for (int p = 0; p < 256; ++p) {
            const int v = ym_aug_mix_blend(a, p, r);
            if (v < 0 || v > 255) return 3;
            out[size_t(a << 8 | p)] = uint8_t(v);
        }
    return write_file(argv[3], out) ? 0 : 2;
}

int main(int argc, char** argv) {
    if ((argc == 6 || argc == 7) && !strcmp(argv[1], "render")) return render(argc, argv);
    if (argc == 4 && !strcmp(argv[1], "blend")) return blend(argv);
    fprintf(stderr, "usage: %s render cases.bin mix.bin out.bin ch [colour.bin] | blend ratio out.bin\n", argv[0]);
    return 2;
}
