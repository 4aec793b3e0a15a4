// VCF replay (vcf_parse.hip): what one lane -- or the host parser's loop body -- does with one data line.
//
// A line of the VCF this program (or Mutation-Simulator 3.0.2, vcf_writer.py:118-126) writes is
//   CHROM \t POS \t ID \t REF \t ALT \t QUAL \t FILTER \t INFO \t FORMAT \t SAMPLE
// Only REF and ALT can be long (a deletion's REF, an inversion's or a duplication's REF and ALT reach megabases), so the
// line is read from both ends: CHROM, POS, ID from the front, SAMPLE, FORMAT, INFO, FILTER, QUAL from the back.  The line
// holds exactly nine tabs (counted by the line-start pass); three are found from the front, five from the back, and
// the position of the ninth -- between REF and ALT -- follows from the record type and the span's length.  The bytes of
// REF and ALT themselves are checked by vcf_long_byte, one call per byte, by whoever owns that byte.
//
// The function is compiled for the host parser and for the device parser alike: one statement of the short fields'
// grammar.  The long parts are written twice (vcf_parse.hip: a sequential loop, a kernel over 16-byte pieces).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msim.h"

namespace msim {

// reasons a line is refused for; the smallest code found on the first offending line is the one reported
enum : uint32_t {
    VCF_OK = 0,
    VCF_R_FIELDS = 1,      // other than 10 tab-separated fields
    VCF_R_LONGFIELD = 2,   // a short field (ID, QUAL, FILTER, INFO, FORMAT) longer than 255 bytes
    VCF_R_POS = 3,         // POS is no number, 0, or beyond the contig
    VCF_R_SAMPLE = 4,      // FORMAT / sample column other than GT / 1
    VCF_R_SVTYPE = 5,      // INFO is neither "." nor SVTYPE=INS|INS:ME|DEL|DEL:ME|INV|DUP
    VCF_R_ALLELE = 6,      // multi-allelic ALT, symbolic allele, breakend
    VCF_R_SNPALT = 7,      // SNP ALT that neither the transition nor a transversion column reaches
    VCF_R_REF = 8,         // REF does not match the genome
    VCF_R_ALT = 9,         // ALT is not what the record type produces from REF
    VCF_R_INSERT = 10,     // an inserted byte that is no letter
    VCF_R_ORDER = 11,      // not behind the input an earlier line consumed
    VCF_R_LENGTH = 12,     // the contig would grow to 2^32 bytes or more
    VCF_R_END = 13,        // consensus grammar: a replacement or insertion that reaches behind the contig's last base
};
constexpr uint32_t VCF_FIELD_CAP = 255;

#define VCF_HD __host__ __device__ inline

// mutator.py:75-77 and the transversion dict of mutator.py:449-455, as code (the device LUT is laid out for the rewrite)
VCF_HD uint8_t vcf_conv(uint8_t b) {
    switch (b) {
        case 'K': return 'G'; case 'S': return 'C'; case 'Y': return 'C'; case 'M': return 'A'; case 'W': return 'A';
        case 'R': return 'A'; case 'B': return 'C'; case 'D': return 'A'; case 'H': return 'A'; case 'V': return 'A';
        case '-': return 'N'; default: return b;
    }
}
VCF_HD uint8_t vcf_comp(uint8_t b) {
    switch (b) {
        case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; case 'U': return 'A';
        case 'M': return 'K'; case 'R': return 'Y'; case 'W': return 'W'; case 'S': return 'S'; case 'Y': return 'R';
        case 'K': return 'M'; case 'V': return 'B'; case 'H': return 'D'; case 'D': return 'H'; case 'B': return 'V';
        default: return b;
    }
}
VCF_HD uint8_t vcf_ti(uint8_t b) {
    switch (b) { case 'A': return 'G'; case 'G': return 'A'; case 'T': return 'C'; case 'C': return 'T'; default: return b; }
}
VCF_HD uint8_t vcf_tv(int col, uint8_t b) {      // 0: the reference raises KeyError
    switch (b) {
        case 'A': return col ? 'C' : 'T'; case 'G': return col ? 'T' : 'C'; case 'T': return col ? 'A' : 'G';
        case 'C': return col ? 'G' : 'A'; case 'N': return 'N'; default: return 0;
    }
}
VCF_HD bool vcf_allele_char(uint8_t b) { return b == ',' || b == '<' || b == '>' || b == '[' || b == ']' || b == '*'; }
VCF_HD bool vcf_letter(uint8_t b) { return (uint8_t)((b | 0x20) - 'a') < 26; }

// what the long-part pass needs to know about a parsed line, in 32 bits
constexpr uint32_t VCF_META_VALID = 1u << 31, VCF_META_LEAD = 1u << 30;
VCF_HD uint32_t vcf_meta(uint32_t r0_rel, uint32_t tail_rel, bool lead) {
    return VCF_META_VALID | (lead ? VCF_META_LEAD : 0u) | (tail_rel << 12) | r0_rel;       // both below 4096
}
VCF_HD uint32_t vcf_meta_r0(uint32_t m) { return m & 4095u; }
VCF_HD uint32_t vcf_meta_tail(uint32_t m) { return (m >> 12) & 4095u; }

struct VcfLine {           // plain scalars, filled once at the end of vcf_parse_line
    uint32_t pos, stop;    // the record's (its extra -- an insert's pool offset -- comes from the scan of ins_len)
    uint32_t type, aux;
    uint32_t ins_len;      // IN: bytes this line adds to the insert pool
    uint32_t meta;
    uint64_t grow;         // bytes this line adds to the contig (IN, DU)
};
VCF_HD msim_record vcf_record(const VcfLine &o, uint32_t extra) {
    msim_record r;
    r.pos = o.pos; r.stop = o.stop; r.extra = extra; r.type = (uint8_t)o.type; r.aux = (uint8_t)o.aux; r.rsv = 0;
    return r;
}

VCF_HD bool vcf_eq(const uint8_t *t, uint64_t at, uint64_t end, const char *lit, uint32_t n) {
    if (end - at != n) return false;
    for (uint32_t i = 0; i < n; i++) if (t[at + i] != (uint8_t)lit[i]) return false;
    return true;
}

// One data line: text bytes [b, e) (no terminator), `tabs` tabs in it, its CHROM `name_len` bytes long (the group's).
// in: the contig's bases (upper-cased), L of them.  Returns VCF_OK and the record, or the reason.
VCF_HD uint32_t vcf_parse_line(const uint8_t *t, uint64_t b, uint64_t e, uint32_t tabs, uint32_t name_len, const uint8_t *in,
                               uint64_t L, VcfLine &o) {
    o.pos = 0; o.stop = 0; o.type = 0; o.aux = 0; o.ins_len = 0; o.meta = 0; o.grow = 0;
    uint32_t r_pos = 0, r_stop = 0, r_type = 0, r_aux = 0, r_ins = 0;
    uint64_t r_grow = 0;
    bool r_lead = false;
    if (tabs != 9) return VCF_R_FIELDS;
    uint64_t p = b + name_len;
    if (p >= e || t[p] != '\t') return VCF_R_FIELDS;
    p++;
    // POS
    uint64_t pos1 = 0;
    uint32_t nd = 0;
    while (p < e && t[p] != '\t') {
        const uint8_t ch = t[p];
        if (ch < '0' || ch > '9' || nd >= 10) return VCF_R_POS;
        pos1 = pos1 * 10 + (ch - '0'); nd++; p++;
    }
    if (nd == 0 || pos1 == 0 || pos1 > L) return VCF_R_POS;
    p++;                                                   // (nine tabs in the line: this one exists)
    // ID
    uint32_t n = 0;
    while (p < e && t[p] != '\t') { if (++n > VCF_FIELD_CAP) return VCF_R_LONGFIELD; p++; }
    const uint64_t r0 = p + 1;
    // from the back: SAMPLE, FORMAT, INFO, FILTER, QUAL
    uint64_t q = e, end[5], beg[5];
    for (int f = 0; f < 5; f++) {
        end[f] = q;
        n = 0;
        while (q > r0 && t[q - 1] != '\t') { if (++n > VCF_FIELD_CAP) return VCF_R_LONGFIELD; q--; }
        if (q <= r0) return VCF_R_FIELDS;                  // (cannot happen with nine tabs; keeps every read inside the line)
        beg[f] = q;
        q--;                                               // the tab in front of the field
    }
    const uint64_t a1 = q;                                 // REF \t ALT = [r0, a1)
    if (a1 < r0 + 3) return VCF_R_ALT;                     // (both non-empty)
    const uint64_t M = a1 - r0;
    if (!vcf_eq(t, beg[0], end[0], "1", 1) || !vcf_eq(t, beg[1], end[1], "GT", 2)) return VCF_R_SAMPLE;
    // INFO
    int kind;                                              // 0 SNP, 1 INS, 2 DEL, 3 INV, 4 DUP
    {
        const uint64_t i0 = beg[2];
        uint64_t i1 = end[2];
        if (vcf_eq(t, i0, i1, ".", 1)) kind = 0;
        else {
            if (i1 - i0 < 10 || !vcf_eq(t, i0, i0 + 7, "SVTYPE=", 7)) return VCF_R_SVTYPE;
            uint64_t s1 = i0 + 7;
            while (s1 < i1 && t[s1] != ';') s1++;
            if (vcf_eq(t, i0 + 7, s1, "INS", 3) || vcf_eq(t, i0 + 7, s1, "INS:ME", 6)) kind = 1;
            else if (vcf_eq(t, i0 + 7, s1, "DEL", 3) || vcf_eq(t, i0 + 7, s1, "DEL:ME", 6)) kind = 2;
            else if (vcf_eq(t, i0 + 7, s1, "INV", 3)) kind = 3;
            else if (vcf_eq(t, i0 + 7, s1, "DUP", 3)) kind = 4;
            else return VCF_R_SVTYPE;
        }
    }
    // alleles this mode does not take: looked for in the first and last 16 bytes of the span (vcf_long_byte sees the rest)
    {
        const uint64_t head = M < 16 ? M : 16;
        for (uint64_t i = 0; i < head; i++) if (vcf_allele_char(t[r0 + i]) || vcf_allele_char(t[a1 - 1 - i])) return VCF_R_ALLELE;
    }
    const uint64_t g0 = pos1 - 1;                          // genome index of REF[0]
    const uint32_t r0_rel = (uint32_t)(r0 - b), tail_rel = (uint32_t)(e - a1);
    switch (kind) {
        case 0: {
            if (M != 3 || t[r0 + 1] != '\t') return VCF_R_ALT;
            const uint8_t ref = t[r0], alt = t[r0 + 2];
            if (ref != vcf_conv(in[g0])) return VCF_R_REF;
            // (selects, not a chain of branches around returns: one exit for the refusal keeps the lanes' control flow flat)
            const uint32_t aux = alt == vcf_ti(ref) ? 0u : alt == vcf_tv(0, ref) ? 1u : alt == vcf_tv(1, ref) ? 2u : 3u;
            if (aux == 3u) return VCF_R_SNPALT;
            r_type = MSIM_SN; r_aux = aux;
            r_pos = (uint32_t)g0; r_stop = (uint32_t)g0;
            break;
        }
        case 1: {                                          // REF one base, ALT = REF + insert | insert + REF
            if (t[r0 + 1] != '\t') return VCF_R_ALT;
            const uint64_t alen = M - 2;
            if (alen < 2) return VCF_R_ALT;
            const uint8_t ref = t[r0];
            if (ref != vcf_conv(in[g0])) return VCF_R_REF;
            bool lead = t[r0 + 2] == ref && pos1 < L;      // (an insert behind the last base is no record: the trailing form, if any)
            if (!lead && t[a1 - 1] != ref) return VCF_R_ALT;
            const uint64_t ilen = alen - 1;
            if (ilen >= (1ull << 32)) return VCF_R_LENGTH;
            r_type = MSIM_IN;
            r_pos = (uint32_t)(lead ? pos1 : g0);
            if ((uint64_t)r_pos + ilen - 1 >= (1ull << 32)) return VCF_R_LENGTH;
            r_stop = (uint32_t)(r_pos + ilen - 1);
            r_ins = (uint32_t)ilen;
            r_grow = ilen;
            r_lead = lead;
            break;
        }
        case 2: {                                          // ALT one base, REF = ALT + deleted | deleted + ALT
            if (t[a1 - 2] != '\t') return VCF_R_ALT;
            const uint64_t R = M - 2;
            if (R < 2) return VCF_R_ALT;
            if (g0 + R > L) return VCF_R_REF;              // REF runs past the contig
            const uint8_t alt = t[a1 - 1];
            const bool lead = t[r0] == alt;
            if (!lead && t[r0 + R - 1] != alt) return VCF_R_ALT;
            r_type = MSIM_DE;
            r_pos = (uint32_t)(lead ? g0 + 1 : g0);
            r_stop = (uint32_t)(r_pos + R - 2);
            r_lead = lead;
            break;
        }
        case 3: {                                          // ALT = reverse complement of REF
            if ((M & 1) == 0) return VCF_R_ALT;
            const uint64_t R = (M - 1) / 2;
            if (t[r0 + R] != '\t') return VCF_R_ALT;
            if (g0 + R > L) return VCF_R_REF;
            r_type = MSIM_IV;
            r_pos = (uint32_t)g0;
            r_stop = (uint32_t)(g0 + R - 1);
            break;
        }
        default: {                                         // ALT = REF REF
            if ((M - 1) % 3 != 0) return VCF_R_ALT;
            const uint64_t R = (M - 1) / 3;
            if (t[r0 + R] != '\t') return VCF_R_ALT;
            if (g0 + R > L) return VCF_R_REF;
            r_type = MSIM_DU;
            r_pos = (uint32_t)g0;
            r_stop = (uint32_t)(g0 + R - 1);
            r_grow = R;
            break;
        }
    }
    o.pos = r_pos; o.stop = r_stop; o.type = r_type; o.aux = r_aux; o.ins_len = r_ins; o.grow = r_grow;
    o.meta = vcf_meta(r0_rel, tail_rel, r_lead);
    return VCF_OK;
}

// check_record_table's rule between neighbours (msim_api.hip): a record starts behind the input its predecessor consumed
VCF_HD uint64_t vcf_next_free(const msim_record &r) {
    return (r.type == MSIM_DE || r.type == MSIM_DU || r.type == MSIM_IV) ? (uint64_t)r.stop + 1 : (uint64_t)r.pos + 1;
}

// One byte of a parsed line's REF \t ALT span: k = its index in the span of M bytes, ch the byte.  Returns the reason it is
// refused for, or VCF_OK; *pool_at >= 0: the byte is an inserted one and belongs at that index of the line's insert.
VCF_HD uint32_t vcf_long_byte(const msim_record &r, bool lead, uint64_t M, uint64_t k, uint8_t ch, const uint8_t *in,
                              int64_t *pool_at) {
    *pool_at = -1;
    uint8_t want;
    bool in_ref;
    switch (r.type) {
        case MSIM_IN: {
            if (k < 2) return VCF_OK;                      // REF and the tab: the lane's
            const uint64_t j = k - 2, alen = M - 2;
            if (lead ? j == 0 : j == alen - 1) return VCF_OK;   // the anchor: the lane's
            if (!vcf_letter(ch)) return vcf_allele_char(ch) ? VCF_R_ALLELE : VCF_R_INSERT;
            *pool_at = (int64_t)(lead ? j - 1 : j);
            return VCF_OK;
        }
        case MSIM_DE: {
            const uint64_t R = M - 2;
            if (k >= R) return VCF_OK;                     // the tab and ALT: the lane's
            want = vcf_conv(in[(lead ? (uint64_t)r.pos - 1 : (uint64_t)r.pos) + k]);
            in_ref = true;
            break;
        }
        case MSIM_IV: {
            const uint64_t R = (M - 1) / 2;
            if (k == R) return VCF_OK;
            in_ref = k < R;
            want = in_ref ? vcf_conv(in[(uint64_t)r.pos + k]) : vcf_comp(vcf_conv(in[(uint64_t)r.stop - (k - R - 1)]));
            break;
        }
        case MSIM_DU: {
            const uint64_t R = (M - 1) / 3;
            if (k == R) return VCF_OK;
            in_ref = k < R;
            uint64_t j = in_ref ? k : k - R - 1;
            if (j >= R) j -= R;
            want = in[(uint64_t)r.pos + j];
            break;
        }
        default: return VCF_OK;                            // SNP: the lane's
    }
    if (ch == want) return VCF_OK;
    return vcf_allele_char(ch) ? VCF_R_ALLELE : (in_ref ? VCF_R_REF : VCF_R_ALT);
}

// ---- the consensus grammar (msim_vcf_select(ctx, 1, sample, haplotype)) ----------------------------------------------------
// Any VCF: the line's selected sample names one of the ALTs (or none: the line is skipped), and REF -> that ALT is decomposed
// into at most a DE and an IN behind it.  Three statements, shared by the host loop and the device kernels:
//   vcf_cons_ends   the short fields from the front, the sample columns, FORMAT, INFO, FILTER, QUAL from the back: POS, where REF
//                   starts, where the ALT field ends, the allele the genotype selects
//   vcf_cons_line   with the REF / ALT separator known: the selected ALT, the anchor, the records' shape
//   vcf_cons_ref_byte / vcf_cons_alt_byte   one byte of REF / of the selected ALT
// No statement walks more than VCF_CONS_WALK bytes of a REF or ALT.
constexpr uint64_t VCF_CONS_WALK = 4096;                   // an ALT field longer than this is taken as one allele (a comma in it: refused)
constexpr uint32_t VCF_C_ALT = 1u, VCF_C_REF = 2u;         // VcfCons::flags: whose bytes the per-byte pass looks at

struct VcfCons {           // one line's state between the steps (the device keeps an array of them)
    uint64_t r0, sep, a1;  // REF = [r0, sep), the ALT field = [sep + 1, a1)
    uint64_t s0;           // the selected ALT = [s0, s0 + A)
    uint32_t pos1, k;      // POS; the selected allele (0: the line is skipped)
    uint32_t g0, R, A;     // genome index of REF[0], the lengths
    uint32_t at, dlen;     // DE [at, at + dlen - 1] (dlen 0: none)
    uint32_t ilen, ioff;   // IN of ALT[ioff, ioff + ilen) in front of base at + dlen (ilen 0: none)
    uint32_t nrec, snp;    // records the line emits; snp: 1 + aux of its SN record (then dlen = ilen = 0)
    uint32_t flags, poff;  // VCF_C_*; the insert's place in the pool
};

VCF_HD uint8_t vcf_upper(uint8_t b) { return (uint8_t)(b - 'a') < 26 ? (uint8_t)(b - 32) : b; }
VCF_HD bool vcf_symbolic(uint8_t b) { return b == '<' || b == '>' || b == '[' || b == ']' || b == ','; }

// nf0: fields of the file's first data line (every line must have as many); sample: 0-based sample column; hap: 1-based entry
VCF_HD uint32_t vcf_cons_ends(const uint8_t *t, uint64_t b, uint64_t e, uint32_t tabs, uint32_t name_len, uint32_t nf0, uint32_t sample,
                              uint32_t hap, uint64_t L, VcfCons &o) {
    o.r0 = o.sep = o.a1 = o.s0 = 0; o.pos1 = o.k = o.g0 = o.R = o.A = o.at = o.dlen = o.ilen = o.ioff = o.nrec = o.snp = o.flags = o.poff = 0;
    if (tabs + 1 != nf0 || !(nf0 == 8 || nf0 >= 10)) return VCF_R_FIELDS;
    uint64_t p = b + name_len;
    if (p >= e || t[p] != '\t') return VCF_R_FIELDS;
    p++;
    uint64_t pos1 = 0;
    uint32_t nd = 0;
    bool pos_bad = false;
    while (p < e && t[p] != '\t') {
        const uint8_t ch = t[p];
        if (ch < '0' || ch > '9' || nd >= 10) pos_bad = true;
        else { pos1 = pos1 * 10 + (ch - '0'); nd++; }
        p++;
    }
    if (nd == 0 || pos1 == 0 || pos1 > L) pos_bad = true;
    p++;
    while (p < e && t[p] != '\t') p++;                     // ID: whatever it holds
    const uint64_t r0 = p + 1;
    // from the back: the sample columns, FORMAT, INFO, FILTER, QUAL -- fields nf0 - 1 down to 5
    uint64_t q = e, gt0 = 0, gt1 = 0, fm0 = 0, fm1 = 0;
    for (uint32_t f = nf0 - 1; f >= 5; f--) {
        const uint64_t end = q;
        while (q > r0 && t[q - 1] != '\t') q--;
        if (q <= r0) return VCF_R_FIELDS;                  // (cannot happen with the tabs counted; keeps every read inside the line)
        if (f == 9 + sample) { gt0 = q; gt1 = end; }
        if (f == 8) { fm0 = q; fm1 = end; }
        q--;
    }
    if (q < r0) return VCF_R_FIELDS;
    uint32_t k = 1;
    if (nf0 >= 10) {
        if (fm1 - fm0 < 2 || t[fm0] != 'G' || t[fm0 + 1] != 'T' || (fm1 - fm0 > 2 && t[fm0 + 2] != ':')) return pos_bad ? VCF_R_POS : VCF_R_SAMPLE;
        uint64_t g1 = gt0;
        while (g1 < gt1 && t[g1] != ':') g1++;
        // the hap-th entry of [gt0, g1) split at '/' and '|'; a single entry serves every hap
        uint32_t total = 1;
        for (uint64_t x = gt0; x < g1; x++) total += t[x] == '/' || t[x] == '|';
        const uint32_t want = total == 1 ? 1 : hap;
        if (want > total) return pos_bad ? VCF_R_POS : VCF_R_SAMPLE;
        uint32_t cur = 1;
        uint64_t e0 = gt0;
        for (uint64_t x = gt0; x < g1 && cur < want; x++) if (t[x] == '/' || t[x] == '|') { cur++; e0 = x + 1; }
        uint64_t e1 = e0;
        while (e1 < g1 && t[e1] != '/' && t[e1] != '|') e1++;
        if (e1 == e0) return pos_bad ? VCF_R_POS : VCF_R_SAMPLE;
        if (e1 - e0 == 1 && t[e0] == '.') k = 0;
        else {
            if (e1 - e0 > 9) return pos_bad ? VCF_R_POS : VCF_R_SAMPLE;
            k = 0;
            for (uint64_t x = e0; x < e1; x++) {
                if (t[x] < '0' || t[x] > '9') return pos_bad ? VCF_R_POS : VCF_R_SAMPLE;
                k = k * 10 + (t[x] - '0');
            }
        }
    }
    o.k = k;
    if (k == 0) return VCF_OK;                             // skipped: nothing else about the line is looked at
    if (pos_bad) return VCF_R_POS;
    o.pos1 = (uint32_t)pos1; o.r0 = r0; o.a1 = q;
    return VCF_OK;
}

// The line's phase word (msim.h: compare --diploid --phased): 0 not phased, MSIM_PHASE_CONTIG phased without a phase set, else its
// PS.  The sample column and FORMAT are found from the back as vcf_cons_ends finds them; only bytes of [b, e) are read.
// *unreadable: the GT is phased and its PS is neither absent, empty, '.' nor a value in 1 .. 0xFFFFFFFE (the word is then 0).
VCF_HD uint32_t vcf_cons_phase(const uint8_t *t, uint64_t b, uint64_t e, uint32_t tabs, uint32_t nf0, uint32_t sample, bool *unreadable) {
    *unreadable = false;
    if (tabs + 1 != nf0 || nf0 < 10 || sample >= nf0 - 9) return 0;
    uint64_t q = e, gt0 = 0, gt1 = 0, fm0 = 0, fm1 = 0;
    for (uint32_t f = nf0 - 1; f >= 8; f--) {
        const uint64_t end = q;
        while (q > b && t[q - 1] != '\t') q--;
        if (q <= b) return 0;                              // (cannot happen with the tabs counted; keeps every read inside the line)
        if (f == 9 + sample) { gt0 = q; gt1 = end; }
        if (f == 8) { fm0 = q; fm1 = end; }
        q--;
    }
    if (fm1 - fm0 < 2 || t[fm0] != 'G' || t[fm0 + 1] != 'T' || (fm1 - fm0 > 2 && t[fm0 + 2] != ':')) return 0;
    uint64_t g1 = gt0;
    uint32_t bars = 0, slashes = 0;
    for (; g1 < gt1 && t[g1] != ':'; g1++) { bars += t[g1] == '|'; slashes += t[g1] == '/'; }
    if (bars == 0 || slashes != 0) return 0;
    // the index of the key that is exactly PS (the first such key)
    constexpr uint32_t NONE = 0xffffffffu;
    uint32_t key = 0, ps = NONE;
    uint64_t k0 = fm0;
    for (uint64_t x = fm0; x <= fm1; x++) {
        if (x < fm1 && t[x] != ':') continue;
        if (ps == NONE && x - k0 == 2 && t[k0] == 'P' && t[k0 + 1] == 'S') ps = key;
        key++;
        k0 = x + 1;
    }
    if (ps == NONE) return MSIM_PHASE_CONTIG;
    uint32_t cur = 0;
    uint64_t s0 = gt0;
    for (uint64_t x = gt0; x < gt1 && cur < ps; x++) if (t[x] == ':') { cur++; s0 = x + 1; }
    if (cur < ps) return MSIM_PHASE_CONTIG;                // the sample has fewer subfields
    uint64_t s1 = s0;
    while (s1 < gt1 && t[s1] != ':') s1++;
    if (s1 == s0 || (s1 - s0 == 1 && t[s0] == '.')) return MSIM_PHASE_CONTIG;
    uint64_t v = 0;
    bool bad = s1 - s0 > 10;
    for (uint64_t x = s0; x < s1 && !bad; x++) {
        if (t[x] < '0' || t[x] > '9') bad = true;
        else v = v * 10 + (uint64_t)(t[x] - '0');
    }
    if (bad || v < 1 || v > 0xFFFFFFFEull) { *unreadable = true; return 0; }
    return (uint32_t)v;
}

// o.sep is known.  Returns the reason the line is refused for (o.flags still says which bytes the per-byte pass checks: a smaller
// reason found there wins), or VCF_OK with the line's records described in o.
VCF_HD uint32_t vcf_cons_line(const uint8_t *t, const uint8_t *in, uint64_t L, VcfCons &o) {
    if (o.k == 0) return VCF_OK;
    const uint64_t r0 = o.r0, sep = o.sep, a1 = o.a1;
    const uint64_t R = sep - r0, F = a1 - (sep + 1);
    uint64_t s0 = sep + 1, s1 = a1;
    if (F <= VCF_CONS_WALK) {
        uint32_t cur = 1;
        for (uint64_t x = sep + 1; x < a1; x++) {
            if (t[x] != ',') continue;
            if (cur == o.k) { s1 = x; break; }
            cur++; s0 = x + 1;
        }
        if (cur < o.k) { o.k = 0; return VCF_R_ALLELE; }
    } else if (o.k != 1) { o.k = 0; return VCF_R_ALLELE; }
    const uint64_t A = s1 - s0;
    if (A == 0) { o.k = 0; return VCF_R_ALLELE; }
    if (A == 1 && t[s0] == '*') { o.k = 0; return VCF_OK; }       // the allele is missing because of an upstream deletion: skipped
    o.s0 = s0;
    o.flags = VCF_C_ALT;
    const uint64_t g0 = (uint64_t)o.pos1 - 1;
    o.g0 = (uint32_t)g0;
    if (A >= (1ull << 32)) { o.A = 0; o.flags = 0; return VCF_R_LENGTH; }
    o.A = (uint32_t)A;
    if (R == 0 || g0 + R > L) return VCF_R_REF;
    o.R = (uint32_t)R;
    o.flags |= VCF_C_REF;
    const uint8_t rf = vcf_upper(t[r0]), rl = vcf_upper(t[sep - 1]), af = vcf_upper(t[s0]), al = vcf_upper(t[s1 - 1]);
    uint64_t at = g0, dlen = R, ilen = A;
    uint32_t ioff = 0;
    if (R == 1 && A == 1) {
        const uint8_t g = in[g0], c = vcf_conv(g);
        if (af == g) return VCF_OK;
        const bool acgt = c == 'A' || c == 'C' || c == 'G' || c == 'T';
        const uint32_t aux = !acgt ? 3u : af == vcf_ti(c) ? 0u : af == vcf_tv(0, c) ? 1u : af == vcf_tv(1, c) ? 2u : 3u;
        if (aux != 3u) { o.at = (uint32_t)g0; o.snp = 1 + aux; o.nrec = 1; return VCF_OK; }
    } else if (rf == af && !(A > 1 && g0 + R == L)) { at = g0 + 1; dlen = R - 1; ilen = A - 1; ioff = 1; }
    else if (rl == al) { dlen = R - 1; ilen = A - 1; }
    if (ilen && at + dlen == L) return VCF_R_END;
    if (ilen && at + dlen + ilen - 1 >= (1ull << 32)) return VCF_R_LENGTH;
    o.at = (uint32_t)at; o.dlen = (uint32_t)dlen; o.ilen = (uint32_t)ilen; o.ioff = ioff;
    o.nrec = (dlen ? 1u : 0u) + (ilen ? 1u : 0u);
    return VCF_OK;
}

// the line's records, in order, at out[0 .. o.nrec)
VCF_HD void vcf_cons_records(const VcfCons &o, uint32_t poff, msim_record *out) {
    uint32_t n = 0;
    msim_record r;
    r.extra = 0; r.aux = 0; r.rsv = 0;
    if (o.snp) { r.pos = o.at; r.stop = o.at; r.type = MSIM_SN; r.aux = (uint8_t)(o.snp - 1); out[n++] = r; return; }
    if (o.nrec == 0) return;
    if (o.dlen) { r.pos = o.at; r.stop = o.at + o.dlen - 1; r.type = MSIM_DE; out[n++] = r; }
    if (o.ilen) { r.pos = o.at + o.dlen; r.stop = r.pos + o.ilen - 1; r.extra = poff; r.type = MSIM_IN; out[n++] = r; }
}

// REF byte j: either form of the genome's base
VCF_HD uint32_t vcf_cons_ref_byte(const VcfCons &o, uint64_t j, uint8_t ch, const uint8_t *in) {
    const uint8_t u = vcf_upper(ch), g = in[(uint64_t)o.g0 + j];
    return (u == g || u == vcf_conv(g)) ? VCF_OK : VCF_R_REF;
}
// byte j of the selected ALT; *pool_at >= 0: it belongs at that index of the line's insert, as *up
VCF_HD uint32_t vcf_cons_alt_byte(const VcfCons &o, uint64_t j, uint8_t ch, int64_t *pool_at, uint8_t *up) {
    *pool_at = -1;
    if (vcf_symbolic(ch)) return VCF_R_ALLELE;
    if (!vcf_letter(ch)) return VCF_R_INSERT;
    if (j >= o.ioff && j - o.ioff < o.ilen) { *pool_at = (int64_t)(j - o.ioff); *up = vcf_upper(ch); }
    return VCF_OK;
}

VCF_HD const char *vcf_reason_text(uint32_t reason) {
    switch (reason) {
        case VCF_R_FIELDS: return "other than 10 tab-separated fields";
        case VCF_R_LONGFIELD: return "ID, QUAL, FILTER, INFO or FORMAT longer than 255 bytes";
        case VCF_R_POS: return "POS is no number, 0, or beyond the contig";
        case VCF_R_SAMPLE: return "FORMAT and sample column other than GT and 1";
        case VCF_R_SVTYPE: return "INFO is neither . nor SVTYPE=INS, INS:ME, DEL, DEL:ME, INV or DUP";
        case VCF_R_ALLELE: return "multi-allelic ALT, symbolic allele or breakend";
        case VCF_R_SNPALT: return "SNP ALT that neither the transition nor a transversion of REF gives";
        case VCF_R_REF: return "REF does not match the genome";
        case VCF_R_ALT: return "ALT is not what the record type produces from REF";
        case VCF_R_INSERT: return "inserted byte that is no letter";
        case VCF_R_ORDER: return "not behind the input an earlier line consumed (positions increasing, no overlap)";
        case VCF_R_LENGTH: return "mutated length of 2^32 or more";
        case VCF_R_END: return "replacement or insertion that reaches behind the contig's last base";
        default: return "unknown reason";
    }
}

// the consensus grammar's wording where the dialect's does not describe it
VCF_HD const char *vcf_cons_reason_text(uint32_t reason) {
    switch (reason) {
        case VCF_R_FIELDS: return "neither 8 nor 10 or more tab-separated fields, or not as many as the first data line";
        case VCF_R_SAMPLE: return "FORMAT does not start with GT, or a genotype entry that is neither a number nor .";
        case VCF_R_ALLELE: return "allele index beyond the ALTs, symbolic allele, breakend, or multi-allelic ALT longer than 4096 bytes";
        case VCF_R_INSERT: return "ALT byte that is no letter";
        default: return vcf_reason_text(reason);
    }
}

}  // namespace msim
