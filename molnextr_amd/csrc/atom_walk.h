// atom_walk.h — the sequential token walk behind the on-device atom-position scan, the confidences (decoder.hip) and the
// packed molecule tables (graph_pack.hip): one definition, so the three cannot drift apart (internal).
#pragma once
#include "dec_types.h"

namespace mnx {

// The sequential walk of the scan over seq[0, n) (ids staged in LDS): calls emit(k, i0, j) for the k-th atom, whose symbol
// tokens are [i0, j) and whose decoder position is j + 2; returns the number of atoms found (kmax does not bound it).
template <typename Emit>
__device__ __forceinline__ int atom_walk(const int* seq, int n, const unsigned char* fl, const TokenClasses* __restrict__ tc,
                                         Emit emit) {
    const int x0 = tc->x0, y0 = tc->y0, lb = tc->lbracket, rb = tc->rbracket;
    const int iC = tc->id_C, il = tc->id_l, iB = tc->id_B, ir = tc->id_r;
    int i = 0, k = 0;
    while (i < n) {
        const int t = seq[i];
        if (t == 2 || t == 0) break;                                  // <eos> / <pad>
        if (t >= x0) { ++i; continue; }                               // coordinate bins
        if (!(fl[t] & 2)) { ++i; continue; }                          // not an atom token
        int j;
        if (t == lb) {
            j = i + 1;
            while (j < n && seq[j] < x0 && (fl[seq[j]] & 1)) {
                ++j;
                if (seq[j - 1] == rb) break;
            }
        } else if (i + 1 < n && ((t == iC && seq[i + 1] == il) || (t == iB && seq[i + 1] == ir))) {
            j = i + 2;
        } else {
            j = i + 1;
        }
        if (j + 2 < n && seq[j] >= x0 && seq[j] < y0 && seq[j + 1] >= y0) {
            emit(k, i, j);
            ++k;
            i = j + 2;
        } else {
            i = j;
        }
    }
    return k;
}

}  // namespace mnx
