// slice_walk.h -- the device function behind lcd_slice_kernel (digar_kernel.hip) and the slice stage of the pass plan (plan_kernel.hip)
#pragma once
#include <hip/hip_runtime.h>
#include "lcd_types.h"

// collect_noisy_read_info's digar walk (src/align.c:1392-1441), one wavefront per (region, read) pair: which query interval of the read lies over the region,
// and does the read cover the region's ends (a deletion longer than the flank at an end counts as a gap).  The reference walks the list in order and lets a
// later digar overwrite what an earlier one set -- an insertion AT the region's first position is followed by the '=' run that starts there, so the run wins --
// and stops at the first digar that begins behind the region.  Here 64 digars are looked at per step: the stop is the first lane whose digar begins behind the
// region, "later overwrites earlier" is the highest matching lane below it (and of the steps so far), the deletion flags are set-only in the reference and so an OR.
// Called by all 64 lanes of a wavefront; every lane returns the same result.
__device__ __forceinline__ SliceOut lcd_slice_walk(const DigarRec *d, const int nd, const int qlen, const long long reg_beg, const long long reg_end, const int flank,
                                                   const int lane) {
    int rb = 0, re = qlen - 1;
    if (nd > 0) { if (d[0].type == 5) rb = d[0].len; if (d[nd - 1].type == 5) re = d[nd - 1].qi - 1; }
    bool hit_b = false, hit_e = false; int beg_del = 0, end_del = 0;
    for (int base = 0; base < nd; base += 64) {
        const int k = base + lane;
        bool cand = false, stop = false; long long db = 0, de = 0; int op = 0, len = 0, qi = 0;
        if (k < nd) {
            const DigarRec r = d[k];
            op = r.type; len = r.len; qi = r.qi; db = r.pos;
            if (op != 4 && op != 5) {
                de = (op == 8 || op == 7 || op == 2) ? db + len - 1 : db;
                stop = db > reg_end;
                cand = !stop && de >= reg_beg;
            }
        }
        const unsigned long long sm = __ballot(stop);
        const unsigned long long below = sm ? ((1ull << __builtin_ctzll(sm)) - 1ull) : ~0ull; // lanes before the first stop
        const unsigned long long mb = __ballot(cand && db <= reg_beg && de >= reg_beg) & below;
        const unsigned long long me = __ballot(cand && db <= reg_end && de >= reg_end) & below;
        if (mb) {
            const int src = 63 - __builtin_clzll(mb);
            const int sop = __shfl(op, src), sqi = __shfl(qi, src); const long long sdb = __shfl(db, src);
            rb = sop == 2 ? sqi : sqi + (int)(reg_beg - sdb); hit_b = true;
            beg_del |= (__ballot(op == 2 && len > flank) & mb) != 0;
        }
        if (me) {
            const int src = 63 - __builtin_clzll(me);
            const int sop = __shfl(op, src), sqi = __shfl(qi, src); const long long sdb = __shfl(db, src);
            re = sop == 2 ? sqi - 1 : sqi + (int)(reg_end - sdb); hit_e = true;
            end_del |= (__ballot(op == 2 && len > flank) & me) != 0;
        }
        if (sm) break;
    }
    int cover = 0; // LONGCALLD_NOISY_{LEFT,RIGHT}_{COVER,GAP} (src/align.c:1442-1456; lcd_types.h LCD_LEFT_COVER ...)
    if (hit_b && hit_e) cover = (beg_del ? LCD_LEFT_GAP : LCD_LEFT_COVER) | (end_del ? LCD_RIGHT_GAP : LCD_RIGHT_COVER);
    else if (hit_b) cover = beg_del ? LCD_LEFT_GAP : LCD_LEFT_COVER;
    else if (hit_e) cover = end_del ? LCD_RIGHT_GAP : LCD_RIGHT_COVER;
    SliceOut o; o.read_beg = rb; o.read_end = re; o.cover = cover; o.pad = 0;
    return o;
}
