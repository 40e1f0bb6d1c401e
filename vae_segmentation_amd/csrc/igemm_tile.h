// What the persistent tile kernels (igemm_k3b.h, igemm_k3t.h, igemm_k3tw.h, igemm_k3x.h, igemm_k4.h) have in common: the walk over the tile list, a tile's
// coordinates and the host side of their divisions.  One definition each: a launch form calls these, it does not copy them.  Every helper here was admitted
// by tools/isa_diff.py: the kernels compile to the device code they had with the copies (profiles/share_helpers_isa_diff.txt).
#pragma once
#include "igemm.h"

// ---- the tile list ---------------------------------------------------------------------------------------------------------------------------------------
// XCD-aware walk: consecutive workgroup ids land on different XCDs (8, each with its own L2).  XCD x owns the contiguous run
// [x*T/8, (x+1)*T/8) of the tile list and its workgroups deal that run round-robin, so neighbouring tiles share an L2 AND every
// XCD gets the same number of tiles (k3b's first walk gave the remainder T mod G to XCD 0 and 1: their CUs ran 9 tiles against
// 6 elsewhere at 96^3, and the launch took as long as they did).  Identity walk when the grid is not a multiple of 8.
// This workgroup's tiles are t, t + G, ... < t_end.
__device__ __forceinline__ void tile_walk(int total_tiles, int& t, int& t_end, int& G) {
    if (((int)gridDim.x & 7) == 0) {
        const int xcd = (int)blockIdx.x & 7;
        G = (int)gridDim.x >> 3;
        t = (int)(((long long)total_tiles * xcd) >> 3) + ((int)blockIdx.x >> 3);
        t_end = (int)(((long long)total_tiles * (xcd + 1)) >> 3);
    } else { G = (int)gridDim.x; t = (int)blockIdx.x; t_end = total_tiles; }
}

// tile t of the list -> sample and first output voxel of a 4 x YT x XT tile (scalar: t is workgroup-uniform); p.fd_m / p.fd_s from tile_fastdiv_fill()
struct TileCoord { int n, z0, y0, x0; };
template <int YT, int XT>
__device__ __forceinline__ TileCoord tile_coord(const G1Params& p, int t) {
    TileCoord c;
    c.n = fdiv(t, p.fd_m[0], p.fd_s[0]);
    const int tl = t - c.n * p.tiles_per_sample;
    const int tz = fdiv(tl, p.fd_m[1], p.fd_s[1]);
    const int r = tl - tz * (p.txn * p.tyn);
    const int ty = fdiv(r, p.fd_m[2], p.fd_s[2]);
    c.z0 = tz * 4; c.y0 = ty * YT; c.x0 = (r - ty * p.txn) * XT;
    return c;
}

// (m, s) with n / d == (mulhi(n, m) + n) >> s for every 0 <= n < 2^31
static inline void tile_fastdiv(int d, unsigned int& m, unsigned int& s) {
    s = 0;
    while ((1ll << s) < d) ++s;
    m = (unsigned int)((((1ull << (32 + s)) + (unsigned long long)d - 1) / (unsigned long long)d) - (1ull << 32));
}
// the three pairs tile_coord divides with, once p.tiles_per_sample, p.txn and p.tyn are final
static inline void tile_fastdiv_fill(G1Params& p) {
    tile_fastdiv(p.tiles_per_sample, p.fd_m[0], p.fd_s[0]);
    tile_fastdiv(p.txn * p.tyn, p.fd_m[1], p.fd_s[1]);
    tile_fastdiv(p.txn, p.fd_m[2], p.fd_s[2]);
}
