// Host harness of synergynet_amd/csrc/face_tables.h -- the very header the kernels of face_tables.hip compile -- for
// tests/test_face_tables_cpu.py.  Build it with clang (hipcc in host mode): the header switches floating-point contraction off with
// a clang pragma.
//   harness sides <sides.i32> <n> <out>   : out = ofs int32 [n,120] | coef int16 [n,120,8]
//   harness boxes <dets.f32>  <n> <out>   : out = roi float32 [n,5] | box int32 [n,4] | w, h int32 [n,2] | status int32 [n]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../synergynet_amd/csrc/face_tables.h"

template <class T>
static bool read_all(const char *path, std::vector<T> &v) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    const bool ok = fread(v.data(), sizeof(T), v.size(), f) == v.size();
    fclose(f);
    return ok;
}

template <class T>
static bool put(FILE *f, const std::vector<T> &v) {
    return fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const long n = atol(argv[3]);
    if (n < 1) return 2;
    FILE *out = fopen(argv[4], "wb");
    if (!out) return 3;
    bool ok = false;
    if (!strcmp(argv[1], "sides")) {
        std::vector<int> sides((size_t)n), ofs((size_t)n * syn::kFtDst);
        std::vector<int16_t> coef((size_t)n * syn::kFtDst * 8);
        if (!read_all(argv[2], sides)) return 3;
        for (long i = 0; i < n; ++i)
            for (int dx = 0; dx < syn::kFtDst; ++dx)
                syn::ft_lanczos4_tap(sides[i], dx, &ofs[i * syn::kFtDst + dx], &coef[(i * syn::kFtDst + dx) * 8]);
        ok = put(out, ofs) && put(out, coef);
    } else if (!strcmp(argv[1], "boxes")) {
        std::vector<float> dets((size_t)n * 5), roi((size_t)n * 5);
        std::vector<int> box((size_t)n * 4), wh((size_t)n * 2), status((size_t)n);
        if (!read_all(argv[2], dets)) return 3;
        for (long i = 0; i < n; ++i) status[i] = syn::ft_roi_box(&dets[i * 5], &roi[i * 5], &box[i * 4], &wh[i * 2], &wh[i * 2 + 1]);
        ok = put(out, roi) && put(out, box) && put(out, wh) && put(out, status);
    }
    return fclose(out) == 0 && ok ? 0 : 4;
}
