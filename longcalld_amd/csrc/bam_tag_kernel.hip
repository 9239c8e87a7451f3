// bam_tag_kernel.hip -- the HP:i / PS:i rewrite of write_read_to_bam (src/bam_utils.c:1944-2006) on the records where the inflate left them in HBM:
//   lcd_bam_tag_measure_kernel  one lane per record: hops the auxiliary fields exactly as lcd_bam_nm_kernel / lcd_bam_aux_kernel do (a field that runs past the
//                               record ends the walk, what lies behind it does not exist), finds the FIRST HP and the FIRST PS field, decides per tag keep /
//                               delete / append and leaves the record's new length;
//   lcd_bam_tag_emit_kernel     one wavefront per record, after the host's prefix sum of the lengths: the record's bytes without the deleted fields, copied
//                               cooperatively (records sit at any byte offset and are tens of kilobytes long), then the appended HP:i, then PS:i, and the new
//                               block_size.
// bam_aux2i is the project's documented rule: types c C s S i I give their value as a 64-bit integer, any other type gives 0.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lcd_types.h"
#include "lcd_kernels.h"
#include "wave_copy.h"
#include "bam_aux_hop.h"

namespace {
using lcd_wave::ld32u;
using lcd_aux::lane_find_nul;   // (the aux hop is shared with bam_refine_kernel.hip: bam_aux_hop.h)
using lcd_aux::aux2i;
} // namespace

__global__ void __launch_bounds__(64) lcd_bam_tag_measure_kernel(const BamTagJob *jobs, BamTagOut *outs, const int n_jobs) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_jobs) return;
    const BamTagJob j = jobs[i];
    const uint8_t *src = (const uint8_t *)(uintptr_t)j.src, *r = src + 4, *end = src + j.len;
    const unsigned w2 = ld32u(r + 8), w3 = ld32u(r + 12);
    const unsigned lname = w2 & 0xff, nc = w3 & 0xffff; const long long lseq = (long long)(int)ld32u(r + 16);
    const uint8_t *aux = r + 32 + lname + 4ull * nc + (unsigned long long)((lseq + 1) / 2) + (unsigned long long)lseq;
    bool have_hp = false, have_ps = false; long long v_hp = 0, v_ps = 0;
    unsigned hp_beg = 0, hp_end = 0, ps_beg = 0, ps_end = 0;
    if (lseq >= 0 && aux <= end)
        while (aux + 3 <= end) {
            const unsigned h = ld32u(aux);
            const uint8_t t0 = (uint8_t)(h & 0xff), t1 = (uint8_t)((h >> 8) & 0xff), ty = (uint8_t)((h >> 16) & 0xff);
            const uint8_t *fld = aux; aux += 3;
            size_t sz = 0; bool bad = false;
            if (ty == 'A' || ty == 'c' || ty == 'C') sz = 1;
            else if (ty == 's' || ty == 'S') sz = 2;
            else if (ty == 'i' || ty == 'I' || ty == 'f') sz = 4;
            else if (ty == 'Z' || ty == 'H') { const long long zl = lane_find_nul(aux, end); if (zl < 0) bad = true; else sz = (size_t)zl + 1; }
            else if (ty == 'B') {
                if (aux + 5 > end) bad = true;
                else {
                    const uint8_t sub = aux[0]; const unsigned cnt = ld32u(aux + 1);
                    const size_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
                    if (!es || (size_t)(end - (aux + 5)) < (size_t)cnt * es) bad = true;
                    else sz = 5 + (size_t)cnt * es;
                }
            } else bad = true;
            if (bad || (size_t)(end - aux) < sz) break;
            if (t0 == 'H' && t1 == 'P' && !have_hp) { have_hp = true; v_hp = aux2i(ty, ld32u(aux)); hp_beg = (unsigned)(fld - src); hp_end = hp_beg + 3u + (unsigned)sz; }
            else if (t0 == 'P' && t1 == 'S' && !have_ps) { have_ps = true; v_ps = aux2i(ty, ld32u(aux)); ps_beg = (unsigned)(fld - src); ps_end = ps_beg + 3u + (unsigned)sz; }
            if (have_hp && have_ps) break;
            aux += sz;
        }
    // per tag: wanted and equal -> stays where it is; wanted otherwise -> the first field (if any) goes and the tag is appended; not wanted -> the first field goes
    const bool want_hp = j.kept && j.hap != 0, want_ps = j.kept && j.ps > 0;
    const bool keep_hp = want_hp && have_hp && v_hp == (long long)j.hap, keep_ps = want_ps && have_ps && v_ps == j.ps;
    BamTagOut o;
    o.flags = (want_hp && !keep_hp ? 1u : 0u) | (want_ps && !keep_ps ? 2u : 0u);
    if (!have_hp || keep_hp) hp_beg = hp_end = 0;
    if (!have_ps || keep_ps) ps_beg = ps_end = 0;
    o.hp_beg = hp_beg; o.hp_end = hp_end; o.ps_beg = ps_beg; o.ps_end = ps_end;
    o.new_len = j.len - (hp_end - hp_beg) - (ps_end - ps_beg) + 7u * ((o.flags & 1u) + ((o.flags >> 1) & 1u));
    o.dst = 0;
    outs[i] = o;
}

__global__ void __launch_bounds__(64) lcd_bam_tag_emit_kernel(const BamTagJob *jobs, const BamTagOut *outs, uint8_t *out, const int n_jobs) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n_jobs) return;
    const BamTagJob j = jobs[i]; const BamTagOut o = outs[i];
    const uint8_t *src = (const uint8_t *)(uintptr_t)j.src;
    uint8_t *dst = out + o.dst;
    // the two deleted fields in record order (an absent one is an empty range at the record's end)
    unsigned a0 = o.hp_end > o.hp_beg ? o.hp_beg : j.len, a1 = o.hp_end > o.hp_beg ? o.hp_end : j.len;
    unsigned b0 = o.ps_end > o.ps_beg ? o.ps_beg : j.len, b1 = o.ps_end > o.ps_beg ? o.ps_end : j.len;
    if (b0 < a0) { const unsigned t0 = a0, t1 = a1; a0 = b0; a1 = b1; b0 = t0; b1 = t1; }
    const unsigned bs = o.new_len - 4u;
    if (lane < 4) dst[lane] = (uint8_t)((bs >> (8 * lane)) & 255u);
    unsigned at = 4;
    lcd_wave::wave_copy(dst + at, src + 4, (long long)a0 - 4, lane); at += a0 - 4;
    lcd_wave::wave_copy(dst + at, src + a1, (long long)b0 - (long long)a1, lane); at += b0 - a1;
    lcd_wave::wave_copy(dst + at, src + b1, (long long)j.len - (long long)b1, lane); at += j.len - b1;
    if (o.flags & 1u) { if (lane < 7) dst[at + lane] = lane == 0 ? 'H' : lane == 1 ? 'P' : lane == 2 ? 'i' : (uint8_t)(((unsigned)j.hap >> (8 * (lane - 3))) & 255u); at += 7; }
    if (o.flags & 2u) { if (lane < 7) dst[at + lane] = lane == 0 ? 'P' : lane == 1 ? 'S' : lane == 2 ? 'i' : (uint8_t)(((unsigned)(unsigned long long)j.ps >> (8 * (lane - 3))) & 255u); }
}

void lcd_launch_bam_tag_measure(const BamTagJob *jobs, BamTagOut *outs, int n_jobs, hipStream_t st) {
    if (n_jobs > 0) hipLaunchKernelGGL(lcd_bam_tag_measure_kernel, dim3((n_jobs + 63) / 64), dim3(64), 0, st, jobs, outs, n_jobs);
}
void lcd_launch_bam_tag_emit(const BamTagJob *jobs, const BamTagOut *outs, uint8_t *out, int n_jobs, hipStream_t st) {
    if (n_jobs > 0) hipLaunchKernelGGL(lcd_bam_tag_emit_kernel, dim3(n_jobs), dim3(64), 0, st, jobs, outs, out, n_jobs);
}
