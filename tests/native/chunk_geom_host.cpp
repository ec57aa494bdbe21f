// Test harness: compiles the slot -> token arithmetic of the fused sliding-chunk attention (esvit_amd/csrc/chunk_geom.h) for the
// HOST so that tests/test_chunk_attn_cpu.py can check it against oracle/ops_ref.chunk_mask without a GPU.  Not part of the library.
#define CG_HD static inline
#include "chunk_geom.h"

extern "C" {
int cg_t_own_slots() { return CG_OWN_SLOTS; }
int cg_t_nb_slots() { return CG_NB_SLOTS; }
int cg_t_max_nglo() { return CG_MAX_NGLO; }
int cg_t_supported(int nglo, int nx, int ny, int w) { return cg_supported(nglo, nx, ny, w); }
int cg_t_chunks(int nglo, int nx, int ny, int w, int* ncx, int* ncy) {
    const ChunkGeom g = cg_make(nglo, nx, ny, w);
    *ncx = g.ncx;
    *ncy = g.ncy;
    return cg_chunks(g);
}
// own[CG_OWN_SLOTS], nb[CG_NB_SLOTS]: the two slot -> token maps of chunk (cr, cc)
void cg_t_maps(int nglo, int nx, int ny, int w, int cr, int cc, int* own, int* nb) {
    const ChunkGeom g = cg_make(nglo, nx, ny, w);
    for (int s = 0; s < CG_OWN_SLOTS; ++s) own[s] = cg_own_token(g, cr, cc, s);
    for (int s = 0; s < CG_NB_SLOTS; ++s) nb[s] = cg_nb_token(g, cr, cc, s);
}
}
