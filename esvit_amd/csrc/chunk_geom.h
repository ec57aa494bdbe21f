// Slot -> token arithmetic of the fused sliding-chunk attention (chunk_attn.hip).
// Tokens of an image are ordered [nglo globals | the nx x ny grid, (x, y) row-major]; a chunk is a w x w tile of the grid, chunk
// (cr, cc) holding x in [w cr, w cr + w) and y in [w cc, w cc + w), both clipped to the grid.  A unit of work is one chunk:
//   own slots            s < w w:  the chunk's tokens, (x - w cr) w + (y - w cc)                            (CG_OWN_SLOTS = 64 slots)
//   neighbourhood slots  s < nglo: the global tokens; then the 3w x 3w square around the chunk, rows of 3w  (CG_NB_SLOTS = 448 slots)
// A slot whose grid position lies outside the grid, and every slot past the last, is dead (-1): the zero padding of the
// reference's sliding-chunk layers is exactly the set of positions that do not exist, so there is nothing to reproduce.
// The neighbourhood is symmetric (query i sees key j <=> key i is seen by query j), so the same two maps serve the forward and dQ
// (own = queries, neighbourhood = keys) and dK / dV (own = keys, neighbourhood = queries).
// Plain C++ (CG_HD expands to __host__ __device__ under hipcc and to nothing under a host compiler): tests/test_chunk_attn_cpu.py
// compiles this header with g++ and checks it against oracle/ops_ref.chunk_mask before any kernel runs.
#pragma once

#ifndef CG_HD
#define CG_HD __host__ __device__ __forceinline__
#endif

constexpr int CG_OWN_SLOTS = 64;   // 4 MFMA tiles of 16
constexpr int CG_NB_SLOTS = 448;   // 14 blocks of 32
constexpr int CG_W = 7;            // the chunk side every yaml of the reference uses
constexpr int CG_MAX_NGLO = CG_NB_SLOTS - 9 * CG_W * CG_W;  // 7

struct ChunkGeom {
    int nglo, nx, ny, w;
    int ncx, ncy;  // chunks per grid side
};

CG_HD ChunkGeom cg_make(int nglo, int nx, int ny, int w) {
    ChunkGeom g;
    g.nglo = nglo;
    g.nx = nx;
    g.ny = ny;
    g.w = w;
    g.ncx = (nx + w - 1) / w;
    g.ncy = (ny + w - 1) / w;
    return g;
}

// 1 if the geometry fits the slot counts above
CG_HD int cg_supported(int nglo, int nx, int ny, int w) {
    return w > 0 && nx > 0 && ny > 0 && nglo >= 0 && w * w <= CG_OWN_SLOTS && nglo + 9 * w * w <= CG_NB_SLOTS;
}

CG_HD int cg_chunks(const ChunkGeom& g) { return g.ncx * g.ncy; }

// own slot s of chunk (cr, cc) -> token of the image, or -1
CG_HD int cg_own_token(const ChunkGeom& g, int cr, int cc, int s) {
    if (s < 0 || s >= g.w * g.w) return -1;
    const int x = cr * g.w + s / g.w, y = cc * g.w + s % g.w;
    if (x >= g.nx || y >= g.ny) return -1;
    return g.nglo + x * g.ny + y;
}

// neighbourhood slot s of chunk (cr, cc) -> token of the image, or -1
CG_HD int cg_nb_token(const ChunkGeom& g, int cr, int cc, int s) {
    if (s < 0) return -1;
    if (s < g.nglo) return s;
    const int t = s - g.nglo, w3 = 3 * g.w;
    if (t >= w3 * w3) return -1;
    const int x = (cr - 1) * g.w + t / w3, y = (cc - 1) * g.w + t % w3;
    if (x < 0 || y < 0 || x >= g.nx || y >= g.ny) return -1;
    return g.nglo + x * g.ny + y;
}
