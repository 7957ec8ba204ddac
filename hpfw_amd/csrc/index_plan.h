// index_plan.h -- the host side of removing clips from the index in place (k_index.hip): the new
// offsets, the moves that close the surviving hashprints up, and their split into the chunks the kernels run.  Plain C++
// (no HIP): tests/emu/index_plan_check.cpp builds it alone.
//
// The rule.  Clips keep their ids; a removed clip becomes empty; the hashprints of the others keep their order and lie back
// to back.  A maximal run of surviving hashprints behind the first removed one is a move (dst, src, len) with src > dst;
// the shift src - dst is the hashprints removed in front of the run, so it never decreases along the list, and the
// destinations of consecutive moves are adjacent.  Nothing in front of the first removed hashprint is touched.
//
// The order, which is the whole correctness argument.  The destination range [d0, d1) of all moves is cut into chunks of at
// most `chunk` hashprints, and the chunks run in ascending order, each after the one before has finished (launch order on
// one stream).  Take the chunk of destinations [a, b):
//   - its sources lie at or to the right of a: every move goes left;
//   - the chunks before it wrote below a only, so its sources still hold the old index;
//   - the chunks behind it read sources at or above their own destinations, which are at or above b, so what this chunk
//     writes into [a, b) is read by none of them.
// What is left is the chunk against itself.  If its first (lowest) source is at or above b, no source meets [a, b): the chunk
// is DIRECT, one launch, and its elements may move in any order.  Otherwise it is STAGED: one launch reads all its sources
// into the staging buffer, the next writes [a, b) from there.  No workgroup ever waits for another.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/hpfw_gpu.h"

namespace hpfw {

constexpr int kIndexTile = 4096;                          // hashprints of the destination one workgroup takes (32 KiB)
// hashprints of a chunk: 128 MiB of staging, the smallest at which the front removal of 18.6 GB is as fast as it gets -- and
// half of the Infinity Cache, from which the second launch of a staged chunk reads what the first wrote
constexpr int64_t kIndexChunkDefault = (int64_t)1 << 24;

// off [n_clips + 1] non-decreasing; removed [n_removed] strictly ascending ids in [0, n_clips); chunk >= 1.
// new_off [n_clips + 1] (may be NULL) receives the offsets after the removal; `moves` (may be NULL) the pieces of the moves,
// chunk after chunk, destinations ascending and adjacent.  false: an argument breaks the conditions above.
inline bool index_remove_plan(const int64_t *off, int64_t n_clips, const int64_t *removed, int64_t n_removed, int64_t chunk,
                              int64_t *new_off, std::vector<hpfw_index_move> *moves)
{
    if (!off || n_clips < 0 || n_removed < 0 || (n_removed > 0 && !removed) || chunk < 1) return false;
    for (int64_t c = 0; c < n_clips; ++c)
        if (off[c + 1] < off[c]) return false;
    for (int64_t r = 0; r < n_removed; ++r)
        if (removed[r] < 0 || removed[r] >= n_clips || (r > 0 && removed[r] <= removed[r - 1])) return false;
    if (moves) moves->clear();
    if (new_off) new_off[0] = off[0];
    // the runs: maximal stretches of surviving hashprints under one non-zero shift
    std::vector<hpfw_index_move> runs;
    int64_t shift = 0, r = 0;
    for (int64_t c = 0; c < n_clips; ++c) {
        const int64_t len = off[c + 1] - off[c];
        if (r < n_removed && removed[r] == c) {
            shift += len;
            ++r;
        } else if (shift > 0 && len > 0) {
            if (!runs.empty() && runs.back().src + runs.back().len == off[c])
                runs.back().len += len; // (only empty clips were removed in between: the shift is the same)
            else
                runs.push_back({off[c] - shift, off[c], len, 0, 0, 0});
        }
        if (new_off) new_off[c + 1] = off[c + 1] - shift;
    }
    if (!moves || runs.empty()) return true;
    // the pieces: a run is cut where its destination crosses a chunk's end
    const int64_t d0 = runs.front().dst;
    for (const hpfw_index_move &m : runs) {
        for (int64_t done = 0; done < m.len;) {
            const int64_t k = (m.dst + done - d0) / chunk;
            const int64_t room = d0 + (k + 1) * chunk - (m.dst + done);
            const int64_t n = m.len - done < room ? m.len - done : room;
            moves->push_back({m.dst + done, m.src + done, n, k, 0, 0});
            done += n;
        }
    }
    // a chunk whose lowest source lies below the end of its destinations is staged
    for (size_t i = 0; i < moves->size();) {
        size_t j = i;
        while (j < moves->size() && (*moves)[j].chunk == (*moves)[i].chunk) ++j;
        const int64_t end = (*moves)[j - 1].dst + (*moves)[j - 1].len;
        const int32_t staged = (*moves)[i].src < end;
        for (; i < j; ++i) (*moves)[i].staged = staged;
    }
    return true;
}

} // namespace hpfw
