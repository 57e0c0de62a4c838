// Host driver of tests/test_pivot_push_host.py: runs the pivot push's index
// math (conflux_amd/csrc/pivot_push.hpp) on cases read from a file.  No GPU
// code.
//
//   pivot_push_host_main <in> <out>
// in:  binary int32; ncases, then per case Ml, M, f, cnt, pos[cnt], gri[Ml]
// out: binary int32; per case status, n_early, n_late, early[cnt], late[cnt]
//      (entries past the counts are -1), gri[Ml], igri[M]
//
// igri is built here as the inverse of gri (-1 on rows not held).  Every
// array has exactly the size the header is promised, each in an allocation
// of its own, so that a sanitizer build sees any write past it; the maps are
// updated only when the lists were accepted, as the engine does.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pivot_push.hpp"

static bool get(FILE *f, std::vector<int32_t> &v) {
    return v.empty() || std::fread(v.data(), 4, v.size(), f) == v.size();
}
static bool put(FILE *f, const std::vector<int32_t> &v) {
    return v.empty() || std::fwrite(v.data(), 4, v.size(), f) == v.size();
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::vector<int32_t> head(1);
    if (!get(in, head)) return 2;
    for (int c = 0, ncases = head[0]; c < ncases; ++c) {
        std::vector<int32_t> h(4);
        if (!get(in, h) || h[0] <= 0 || h[1] < h[0] || h[3] < 0) return 2;
        const int Ml = h[0], M = h[1], f = h[2], cnt = h[3];
        std::vector<int32_t> pos(cnt), gri(Ml), igri(M, -1);
        if (!get(in, pos) || !get(in, gri)) return 2;
        for (int i = 0; i < Ml; ++i) {
            if (gri[i] < 0 || gri[i] >= M) return 2;
            igri[gri[i]] = i;
        }
        std::vector<int32_t> early(cnt, -1), late(cnt, -1), res(3);
        int n_early = 0, n_late = 0;
        res[0] = pivot_push::lists(pos.data(), cnt, f, Ml, early.data(),
                                   late.data(), &n_early, &n_late);
        res[1] = n_early;
        res[2] = n_late;
        if (res[0] == pivot_push::OK)
            pivot_push::apply(gri.data(), igri.data(), pos.data(), cnt, f,
                              early.data(), late.data(), n_late);
        for (int i = n_early; i < cnt; ++i) early[i] = -1;
        for (int i = n_late; i < cnt; ++i) late[i] = -1;
        if (!put(out, res) || !put(out, early) || !put(out, late) ||
            !put(out, gri) || !put(out, igri))
            return 2;
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 2;
}
