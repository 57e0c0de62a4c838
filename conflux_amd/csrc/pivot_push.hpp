// pivot_push.hpp — host index math of the pivot push (step 2 of the LU
// superstep).  No HIP, no engine types: plain pointers, so it is tested on
// the CPU (tests/test_pivot_push_host.py).
//
// A rank row holds Ml local rows; rows [0, f) are retired, [f, Ml) active.
// A step's cnt pivot rows sit at the local positions pos[0..cnt) and must end
// up, in that order, in the window [f, f + cnt).  The kernels do it in three
// moves per matrix:
//   1. gather the pivot rows pos[i] into a staging buffer,
//   2. copy each early row (a window row that is not a pivot) to the matching
//      late position (a pivot row's position beyond the window),
//   3. place the staged pivot rows at [f, f + cnt).
// lists() produces early and late; apply() does the same three moves on the
// host maps gri (global row at each local position) and igri (its inverse on
// the rows this rank row owns).  Work is O(cnt log cnt), not O(Ml).
#pragma once
#include <algorithm>
#include <vector>

namespace pivot_push {

enum { OK = 0, ERANGE_POS = 1, EINVARIANT = 2 };

// early[0..*n_early) ascending, late[0..*n_late) ascending and unique; both
// arrays hold cnt entries.  Returns ERANGE_POS when the window or a position
// leaves [0, Ml) (nothing is written then), EINVARIANT when the counts differ
// (a repeated or an already retired row); the counts are set either way.
inline int lists(const int *pos, int cnt, int f, int Ml, int *early, int *late,
                 int *n_early, int *n_late) {
    *n_early = *n_late = 0;
    if (cnt < 0 || f < 0 || f + cnt > Ml) return ERANGE_POS;
    for (int i = 0; i < cnt; ++i)
        if (pos[i] < 0 || pos[i] >= Ml) return ERANGE_POS;
    // only positions [f, f+cnt) and the pivot rows' own positions matter
    std::vector<char> in_win(cnt, 0);
    int ne = 0, nl = 0;
    for (int i = 0; i < cnt; ++i) {
        const int p = pos[i];
        if (p >= f && p < f + cnt)
            in_win[p - f] = 1;
        else if (p >= f + cnt)
            late[nl++] = p;
    }
    std::sort(late, late + nl);
    nl = (int)(std::unique(late, late + nl) - late);
    for (int i = 0; i < cnt; ++i)
        if (!in_win[i]) early[ne++] = f + i;
    *n_early = ne;
    *n_late = nl;
    return ne == nl ? OK : EINVARIANT;
}

// the three moves on gri / igri, for lists that lists() accepted
inline void apply(int *gri, int *igri, const int *pos, int cnt, int f,
                  const int *early, const int *late, int n_late) {
    std::vector<int> tmp(cnt);
    for (int i = 0; i < cnt; ++i) tmp[i] = gri[pos[i]];
    for (int i = 0; i < n_late; ++i) {
        gri[late[i]] = gri[early[i]];
        igri[gri[late[i]]] = late[i];
    }
    for (int i = 0; i < cnt; ++i) {
        gri[f + i] = tmp[i];
        igri[tmp[i]] = f + i;
    }
}

}  // namespace pivot_push
