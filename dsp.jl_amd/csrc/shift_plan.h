// shiftsignal / shiftsignal! (src/util.jl:357-395): y[i] = x[i - s] where that exists, else 0, for one line of l elements of 4, 8 or 16 bytes.
// The planner, the HALO schedule and a host emulation that runs the same schedule; the kernels are shift.hip.
//
// Routes (d = |s|; "in place": y is x):
//   DISJOINT  out of place, or in place with 2 d >= l: the source range ([0, l - d) for s > 0, [d, l) for s < 0) and the destination range do not
//             overlap.  One launch, a thread per destination element.  In place the source range lies inside the range that becomes zero: the thread
//             that reads x[j] is the only one that ever touches word j -- it stores the zero there itself, after its load -- so no word is read after
//             another thread wrote it.
//   HALO      in place, 0 < d < l / 2.  Destination tiles of `tile` >= d elements, a workgroup each.  The sources of tile t are its own elements and d
//             elements of ONE neighbour (the halo: below the tile for s > 0, above it for s < 0).  Launch 1 copies every halo into the workspace;
//             nothing of the line is written in it.  Launch 2: a workgroup walks its tile in chunks -- from the end for s > 0, from the start for
//             s < 0 -- loads a chunk's sources (own tile or workspace), waits until every load has returned, passes a barrier, stores.  The sources of
//             the chunks still to come lie beyond everything stored so far, and no workgroup reads a word of the line outside its own tile.
//   STAGED    HALO would leave fewer tiles than compute units (256 assumed, as everywhere in the planners): the source range is copied to the
//             workspace (launch 1), the DISJOINT kernel reads it from there (launch 2).
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define SHIFT_HD __host__ __device__ inline
#else
#define SHIFT_HD inline
#endif

namespace mdsp {
namespace shiftplan {

enum : int { ROUTE_AUTO = 0, ROUTE_DISJOINT = 1, ROUTE_HALO = 2, ROUTE_STAGED = 3 };
enum : int { PLAN_OK = 0, PLAN_DOMAIN = 1, PLAN_ARGUMENT = 2 };
enum : int { SRC_ZERO = 0, SRC_LINE = 1, SRC_HALO = 2 };

constexpr int64_t TILE_BYTES = 256 << 10;   // default destination tile of the HALO route
constexpr int64_t CHUNK_MAX = 1024;         // elements a workgroup of 256 threads moves between two barriers (four per thread)
constexpr int64_t MIN_TILES = 256;          // fewer HALO tiles than this: STAGED

struct Plan {
    int route = ROUTE_DISJOINT;
    bool in_place = false;
    int64_t l = 0, s = 0, d = 0, esize = 4, tile = 0, chunk = 0, ntiles = 0, workspace = 0;   // workspace in ELEMENTS
};

// s > 0: x[0 .. l-d) moves up; s < 0: x[d .. l) moves down
SHIFT_HD int64_t source_begin(int64_t s, int64_t d) { return s > 0 ? 0 : d; }
// in place, DISJOINT: is word i part of the source range (its reader stores the zero)?
SHIFT_HD bool in_source(int64_t i, int64_t l, int64_t s, int64_t d) { return s > 0 ? i < l - d : i >= d; }

inline int make_plan(int64_t l, int64_t s, int64_t esize, bool in_place, int64_t tile, int route, Plan* out, const char** why) {
    Plan p;
    const int64_t d = s < 0 ? -s : s;
    if (l < 0 || (esize != 4 && esize != 8 && esize != 16) || tile < 0 || route < ROUTE_AUTO || route > ROUTE_STAGED) {
        *why = "shift: length >= 0, elements of 4, 8 or 16 bytes, tile >= 0 (0 = auto), a route of 0 .. 3";
        return PLAN_ARGUMENT;
    }
    if (d > l) {
        *why = "The absolute value of s must not be greater than the length of x";   // util.jl:359-361
        return PLAN_DOMAIN;
    }
    p.in_place = in_place;
    p.l = l;
    p.s = s;
    p.d = d;
    p.esize = esize;
    p.tile = tile > 0 ? tile : TILE_BYTES / esize;
    if (p.tile < d) p.tile = d;
    p.chunk = p.tile / 4 < 16 ? 16 : p.tile / 4;
    if (p.chunk > CHUNK_MAX) p.chunk = CHUNK_MAX;
    p.ntiles = (l + p.tile - 1) / p.tile;
    const bool overlap = in_place && d > 0 && 2 * d < l;
    if (route == ROUTE_AUTO) route = !overlap ? ROUTE_DISJOINT : p.ntiles < MIN_TILES ? ROUTE_STAGED : ROUTE_HALO;
    if (route == ROUTE_DISJOINT && overlap) {
        *why = "shift: the DISJOINT route in place needs 2 |s| >= l (source and destination overlap)";
        return PLAN_ARGUMENT;
    }
    if (route == ROUTE_HALO && !(in_place && d > 0)) {
        *why = "shift: the HALO route is the in-place route for s != 0";
        return PLAN_ARGUMENT;
    }
    p.route = route;
    p.workspace = route == ROUTE_HALO ? p.ntiles * d : route == ROUTE_STAGED ? l - d : 0;
    *out = p;
    return PLAN_OK;
}

// ---- HALO schedule
// halo word h of tile t is line word ... (may lie outside [0, l): then it is never copied and never read)
SHIFT_HD int64_t halo_word(int64_t t, int64_t h, int64_t s, int64_t d, int64_t tile) { return s > 0 ? t * tile - d + h : (t + 1) * tile + h; }
// chunk c of the tile [t0, t1): destination range [*d0, *d1)
SHIFT_HD void chunk_range(int64_t c, int64_t t0, int64_t t1, int64_t s, int64_t chunk, int64_t* d0, int64_t* d1) {
    if (s > 0) {
        *d1 = t1 - c * chunk;
        *d0 = *d1 - chunk > t0 ? *d1 - chunk : t0;
    } else {
        *d0 = t0 + c * chunk;
        *d1 = *d0 + chunk < t1 ? *d0 + chunk : t1;
    }
}
// where destination i of tile t takes its element from: *idx is a word of the line (SRC_LINE) or of the workspace (SRC_HALO)
SHIFT_HD int source_of(int64_t i, int64_t t, int64_t l, int64_t s, int64_t d, int64_t tile, int64_t* idx) {
    const int64_t j = i - s, t0 = t * tile;
    if (j < 0 || j >= l) return SRC_ZERO;
    if (j >= t0 && j < t0 + tile) {
        *idx = j;
        return SRC_LINE;
    }
    *idx = t * d + (s > 0 ? j - (t0 - d) : j - (t0 + tile));
    return SRC_HALO;
}

// ---- host emulation: the plan's launches one after the other, the units of a launch in the order `order` (0 ascending, 1 descending, 2 odd units
// first).  With y == x every word of the line that is read is checked: *violations counts reads of a word that was already written, and HALO reads of a
// word outside the reader's own tile.
template <typename E> inline void emulate(const Plan& p, const E* x, E* y, int order, int64_t* violations) {
    const bool inpl = static_cast<const void*>(x) == static_cast<void*>(y);
    std::vector<char> written((size_t)(inpl ? p.l : 0), 0);
    std::vector<E> ws((size_t)p.workspace);
    int64_t bad = 0;
    E zero;
    std::memset(&zero, 0, sizeof(E));
    auto read = [&](int64_t j) {
        if (inpl && written[(size_t)j]) ++bad;
        return x[j];
    };
    auto write = [&](int64_t i, E v) {
        y[i] = v;
        if (inpl) written[(size_t)i] = 1;
    };
    auto each = [&](int64_t n, auto&& fn) {
        if (order == 0) for (int64_t k = 0; k < n; ++k) fn(k);
        else if (order == 1) for (int64_t k = n - 1; k >= 0; --k) fn(k);
        else {
            for (int64_t k = 1; k < n; k += 2) fn(k);
            for (int64_t k = 0; k < n; k += 2) fn(k);
        }
    };
    auto disjoint = [&](const E* src, int64_t src_off, bool zero_src) {   // the DISJOINT kernel, a thread per destination
        each(p.l, [&](int64_t i) {
            const int64_t j = i - p.s;
            if (j >= 0 && j < p.l) {
                const E v = src == x ? read(j) : src[j - src_off];
                write(i, v);
                if (zero_src) write(j, zero);
            } else if (!(zero_src && in_source(i, p.l, p.s, p.d))) write(i, zero);
        });
    };
    if (p.route == ROUTE_DISJOINT) {
        if (inpl && p.s == 0) return;
        disjoint(x, 0, inpl);
    } else if (p.route == ROUTE_STAGED) {
        const int64_t b = source_begin(p.s, p.d);
        for (int64_t k = 0; k < p.l - p.d; ++k) ws[(size_t)k] = read(b + k);
        disjoint(ws.data(), b, false);
    } else {
        for (int64_t g = 0; g < p.ntiles * p.d; ++g) {
            const int64_t j = halo_word(g / p.d, g % p.d, p.s, p.d, p.tile);
            if (j >= 0 && j < p.l) ws[(size_t)g] = read(j);
        }
        std::vector<E> v((size_t)p.chunk);
        each(p.ntiles, [&](int64_t t) {
            const int64_t t0 = t * p.tile, t1 = t0 + p.tile < p.l ? t0 + p.tile : p.l;
            for (int64_t c = 0; c * p.chunk < t1 - t0; ++c) {
                int64_t d0, d1, idx = 0;
                chunk_range(c, t0, t1, p.s, p.chunk, &d0, &d1);
                for (int64_t i = d0; i < d1; ++i) {
                    const int kind = source_of(i, t, p.l, p.s, p.d, p.tile, &idx);
                    if (kind == SRC_LINE && (idx < t0 || idx >= t1)) ++bad;
                    v[(size_t)(i - d0)] = kind == SRC_ZERO ? zero : kind == SRC_LINE ? read(idx) : ws[(size_t)idx];
                }
                for (int64_t i = d0; i < d1; ++i) write(i, v[(size_t)(i - d0)]);
            }
        });
    }
    if (violations) *violations = bad;
}

}  // namespace shiftplan
}  // namespace mdsp
