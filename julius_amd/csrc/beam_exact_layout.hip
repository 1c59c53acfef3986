// beam_exact_layout.hip -- the LDS image of the exact-order kernels (beam_exact.hip, beam_exact_mp.h), laid out on the
// host: xbeam_layout() when a work area is created (beam_api.hip), xbeam_place() for the per-launch part
// (xbeam_launch()).  Plain C++: the kernels see the result as byte offsets in XWork (beam_exact.h).
#include "beam_exact.h"

namespace jamdb {

// The fixed part of the image for one of the two layouts.
//   narrow: [survivors Tok[beam]] [atom] [welist] [dbase] [tpre] [bitmap] | cells / pruning overlay | score row
//   wide:   [welist] | [atom] [dbase] [tpre] [bitmap] cells | score row     -- the survivors live in the utterance's
//           slice (o_sv: steps 0 and A read them in order, only the winner look-ups of step C are gathers), and the
//           pruning step overlays everything behind welist[] (all of it is dead between step C and the next step 0;
//           welist[] carries the pruning step's result).
static int xbeam_fixed(XWork *xw, bool wide, int maxfan, int nroot, int ninit, int nshared) {
  const int beam = xw->w.beam;
  int at = 0;
  auto place = [&](int *off, int bytes) { *off = at; at = (at + bytes + 15) & ~15; };
  xw->wide = wide ? 1 : 0;
  if (!wide) {
    at = beam * (int)sizeof(Tok);
    place(&xw->off_atom, 4 * beam);
    place(&xw->off_we, 4 * beam);
    place(&xw->off_dbase, 4 * (beam + 2));
    xw->w.sv_bytes = at;                             // what a streaming session parks between launches
    place(&xw->off_tpre, 4 * xw->nt);
  } else {
    place(&xw->off_we, 4 * beam);
    xw->off_dov = at;
    place(&xw->off_atom, 4 * beam);
    place(&xw->off_dbase, 4 * (beam + 2));
    xw->w.sv_bytes = (beam * (int)sizeof(Tok) + 15) & ~15;   // the survivors' home in the slice; nothing to park
    place(&xw->off_tpre, 4 * xw->nt);
  }
  if (at + 8 * 1024 > xw->lds_budget) return -2;
  // creation-order bitmap: XW bits per source plus a few word ends' worth of roots (a frame that needs more
  // uses the copy in global memory); at most an eighth of what is left
  int bm_words = (beam * maxfan + 8 * nroot + nshared + ninit + 31) / 32 + 64;
  if (bm_words > 4096) bm_words = 4096;
  if (4 * bm_words > (xw->lds_budget - at) / 8) bm_words = (xw->lds_budget - at) / 32;
  xw->bm_words = bm_words;
  place(&xw->off_bm, 4 * bm_words);
  xw->cells_at = at;
  if (!wide) xw->off_dov = at;
  return 0;
}

static int xbeam_tail_bytes(int beam) {
  return (4 * ((beam + 31) / 32 + 2 + 4 * kMaxCand + 4 + (kMaxCand + 1) * (kTakers + 1)) + 15) & ~15;
}

// The per-launch part with `want` bytes set aside for the score row.  The frame's Viterbi cells take what is left
// (16 bytes a slot); the pruning step overlays them (narrow) or everything behind welist[] (wide):
//   narrow: [compR|compT 16 b_cap] [vposR 4] [idR 4] [hist] [tail] [heap: the rest]
//   wide:   [compA|compB 16 b_cap] [idA 4] [idB 4] ... [hist] [tail]   with the heap laid over the lists (it is dead
//           once the top elements are collected into o_collect) and vposR over compA (dead once the list is sorted)
// b_cap = 0: no room for the closed-form extraction (the sequential extraction runs on one lane).
static void xbeam_place_with(XWork *xw, int want) {
  const int beam = xw->w.beam;
  const int cells_at = xw->cells_at;
  int region = ((xw->lds_budget - cells_at) & ~1023) - want;
  if (region < 0) region = 0;
  int nslot = (region / 16) & ~63;
  if (nslot < 1024) nslot = 0;                       // too few to be worth probing: every cell in nodekey[]
  xw->nslot = nslot;
  xw->off_cells = cells_at;
  xw->off_lnode = cells_at + 8 * nslot;
  xw->off_lfirst = cells_at + 12 * nslot;
  const int end = cells_at + region;
  const int tail_bytes = xbeam_tail_bytes(beam);
  int at = xw->off_dov;
  auto place = [&](int *off, int bytes) { *off = at; at = (at + bytes + 15) & ~15; };
  xw->b_cap = beam + 256;
  if (!xw->wide) {
    if (16 * xw->b_cap + 8 * xw->b_cap + 4 * 2048 + tail_bytes + 128 + 8 * (2 * beam + 64) > region) xw->b_cap = 0;
    place(&xw->off_compr, 16 * xw->b_cap);
    place(&xw->off_vpos, 4 * xw->b_cap);
    place(&xw->off_id, 4 * xw->b_cap);
    xw->off_idt = xw->off_id;
    place(&xw->off_hist, xw->b_cap ? 4 * 2048 : 0);
    place(&xw->off_tail, tail_bytes);
    place(&xw->off_heap, 0);
    xw->heap_cap = (end - xw->off_heap) / 8 - 2;
  } else {
    const int dreg = end - xw->off_dov;
    if (24 * xw->b_cap + 4 * 2048 + tail_bytes + 64 > dreg) xw->b_cap = 0;
    xw->off_tail = end - tail_bytes;
    xw->off_hist = xw->off_tail - 4 * 2048;
    xw->off_heap = xw->off_dov;
    place(&xw->off_compr, 16 * xw->b_cap);
    place(&xw->off_idt, 4 * xw->b_cap);
    place(&xw->off_id, 4 * xw->b_cap);
    xw->off_vpos = xw->off_compr;
    xw->heap_cap = (xw->off_hist - xw->off_heap) / 8 - 2;
  }
  if (xw->heap_cap < 0) xw->heap_cap = 0;
  xw->off_row = end;
  xw->lds_bytes = end;
}

void xbeam_place(XWork *xw, int nstate) {
  xbeam_place_with(xw, 0);
  xw->w.row_cache = 0;
  if (nstate <= 0) return;
  // make room for the frame's score row when the cell table, the LDS heap and the top lists can spare it (the half
  // shape asks for the narrow layout's cell count: with half the LDS, cells lost to the row cost more than the row saves)
  XWork t = *xw;
  xbeam_place_with(&t, (4 * nstate + 1023) & ~1023);
  const int beam = xw->w.beam;
  const bool ok = t.b_cap == xw->b_cap && t.off_row + 4 * nstate <= xw->lds_budget &&
                  (xw->wide && xw->nt == NT ? 2 * t.heap_cap >= 5 * beam : (t.nslot >= 6 * beam && t.heap_cap >= 5 * beam));
  if (!ok) return;                                   // the row stays in global memory
  *xw = t;
  xw->w.row_cache = 1;
}

int xbeam_layout(XWork *xw, const Work &w, int maxfan, int nroot, int ninit, int nshared, bool half, bool mp) {
  xw->w = w;
  xw->mp = mp ? 1 : 0;
  xw->nt = half ? kHalfNT : NT;
  xw->lds_budget = half ? kHalfDynLds : kMaxDynLds;
  const int beam = w.beam;
  xw->xw = maxfan;                                   // self, next, extra arcs
  int need = maxfan + nroot;                         // transition numbers of one source
  if (ninit > need) need = ninit;
  if (maxfan + nshared > need) need = maxfan + nshared;
  if (mp) {                                          // second half of a multipath frame: root number * maxfan + the root's transition
    if (nroot * maxfan > need) need = nroot * maxfan;
    if (nshared * maxfan > need) need = nshared * maxfan;
  }
  int s1 = 1; while ((1 << s1) < need + 1) s1++;
  int jb = 1; while ((1 << jb) < beam + 2) jb++;
  if (s1 + jb > 32) return -1;
  xw->s1 = s1;
  if ((long long)w.tok_cap + 2 >= (1ll << (kMaxL + 1))) return -3;   // prekey() numbers heap positions below 2^(kMaxL+1)
  // the narrow layout (survivors in LDS) while it leaves room for the closed-form extraction and for the heap of a
  // typical frame (three to six tokens per survivor) beside the top lists, else the wide one
  int rc = half ? -2 : xbeam_fixed(xw, false, maxfan, nroot, ninit, nshared);   // (the half shape: always the wide layout)
  if (rc == 0) { xbeam_place_with(xw, 0); if (xw->b_cap == 0 || xw->heap_cap < 8 * beam) rc = -2; }
  if (rc != 0) {
    rc = xbeam_fixed(xw, true, maxfan, nroot, ninit, nshared);
    if (rc != 0) return rc;
    xbeam_place_with(xw, 0);
  }
  // the half shape is there for throughput: only where a typical frame still runs out of LDS
  if (half && (xw->b_cap == 0 || xw->heap_cap < 5 * beam || xw->nslot < 3 * beam)) return -2;
  xw->w.row_cache = 0;
  xw->prune_mode = 0;
  return 0;
}

}  // namespace jamdb
