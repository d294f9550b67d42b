// Sam.hpp -- the SAM lines of `real -sam`: the header, where a read finally lies (SamPlace, from the records the
// run holds), and one line for a read, its placement, its mate's placement and its mismatch list (appendSam).  NM and MD are
// written from the list alone: real_hip_mismatch entries in ascending offset, computed on the device (real_hip_mismatches*;
// for a mate the gap rescue placed, real_hip_mismatches_gapped).
// Host code only, in the manner of Lines.hpp: nothing here calls into the library.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "Lines.hpp"
#include "real_hip.h"

// a fragment's SAM name: the first whitespace-delimited token of what the loader keeps of its header line
inline std::string samName(const std::string &fragname)
{
    size_t a = 0;
    while (a < fragname.size() && (fragname[a] == ' ' || fragname[a] == '\t' || fragname[a] == '\r')) ++a;
    size_t e = a;
    while (e < fragname.size() && fragname[e] != ' ' && fragname[e] != '\t' && fragname[e] != '\r') ++e;
    return fragname.substr(a, e - a);
}

// the fragments of all genome files: SAM names, starts in their file's text (n + 1 per file)
struct SamRefs {
    std::vector<std::vector<std::string>> names;
    std::vector<std::vector<uint64_t>> starts;
    SamRefs(const std::vector<std::vector<std::string>> &fragnames, const std::vector<std::vector<uint64_t>> &fragstarts) : starts(fragstarts)
    {
        for (const auto &f : fragnames) {
            names.emplace_back();
            for (const std::string &n : f) names.back().push_back(samName(n));
        }
    }
    std::string header() const
    {
        std::string h = "@HD\tVN:1.6\tSO:unknown\n";
        for (size_t f = 0; f < names.size(); ++f)
            for (size_t k = 0; k < names[f].size(); ++k)
                h += "@SQ\tSN:" + names[f][k] + "\tLN:" + std::to_string(starts[f][k + 1] - starts[f][k]) + "\n";
        return h + "@PG\tID:real\n";
    }
};

// where a read finally lies, from the record that places it
struct SamPlace {
    bool placed = false, inverted = false, paired = false; // paired: the placement is a Unique pair record's
    bool duplicate = false; // -dedup marked the read (the fragment): FLAG 1024
    unsigned file = 0, frag = 0;
    uint64_t pos = 0; // 0-based in the file's text
    float score = 0.f;
    unsigned mapq = REAL_HIP_MAPQ_NONE; // -mapq 1: the placement's mapping quality (real_hip_mapq*); 255: not available
    // -sam_gapped 1: a mate the gap rescue placed (samPlaceGapped) carries its CIGAR, its span on the text, its inserted bases
    // and its cost; `proper` is the fragment's: the outer distance of anchor and rescued mate lies inside the insert bounds
    bool gapped = false, proper = false;
    uint64_t span = 0;
    unsigned inserted = 0, cost = 0;
    char cigar[48] = {0};
};
// single-end: a record of state 1 or 2
inline SamPlace samPlace(const Record &r, float score)
{
    SamPlace p;
    p.placed = r.st == 1 || r.st == 2; p.inverted = r.st == 2;
    p.file = r.file; p.frag = r.frag; p.pos = r.pos; p.score = score;
    return p;
}
// mate 1 (mate = 0) or mate 2 of a fragment: the pair record if it is Unique; else, for a fragment without any concordant
// pair, the mate's own record if that is Unique (the rule -unpaired prints by); a NonUnique pair places nothing
inline SamPlace samPlace(const real_hip_pair &P, const real_hip_single &S, unsigned mate)
{
    SamPlace p;
    if (P.state == REAL_HIP_PAIR_UNIQUE) {
        p.placed = p.paired = true; p.inverted = (P.inverted1 != 0) != (mate != 0);
        p.file = P.fileid; p.frag = P.frag; p.pos = mate ? P.pos2 : P.pos1; p.score = mate ? P.score2 : P.score1;
    } else if (P.state == REAL_HIP_PAIR_NOMATCH && REAL_HIP_SINGLE_STATE(S.tag) == REAL_HIP_PAIR_UNIQUE) {
        p.placed = true; p.inverted = REAL_HIP_SINGLE_INVERTED(S.tag) != 0;
        p.file = S.fileid; p.frag = S.frag; p.pos = S.pos; p.score = S.score;
    }
    return p;
}
// a mate the gap rescue placed: a Unique gap record, for its target mate of `len` bases; cigar: real_hip_gap_cigar's text
inline SamPlace samPlaceGapped(const real_hip_gap_place &g, uint64_t len, const char *cigar)
{
    SamPlace p;
    p.placed = p.gapped = true; p.inverted = REAL_HIP_GAP_INVERTED(g.tag) != 0;
    p.file = g.fileid; p.frag = g.frag; p.pos = g.pos;
    p.span = (uint64_t)((int64_t)len + g.gap); p.inserted = g.gap < 0 ? (unsigned)-g.gap : 0u; p.cost = g.cost;
    snprintf(p.cigar, sizeof p.cigar, "%s", cigar);
    return p;
}
// the outer distance of the insert block of two mates on opposite strands: from the forward mate's first base to the reverse
// mate's last; span_*: what each mate covers of the text (its length; a rescued mate's span)
inline int64_t samOuter(const SamPlace &self, const SamPlace &mate, uint64_t span_self, uint64_t span_mate)
{
    return self.inverted ? (int64_t)(self.pos + span_self) - (int64_t)mate.pos : (int64_t)(mate.pos + span_mate) - (int64_t)self.pos;
}
// TLEN of a mate of a Unique pair: the outer distance of the insert block, positive for the forward mate
inline int64_t samTlen(const SamPlace &self, const SamPlace &mate, uint64_t len_self, uint64_t len_mate)
{
    if (!self.paired) return 0;
    const int64_t outer = samOuter(self, mate, len_self, len_mate);
    return self.inverted ? -outer : outer;
}

inline void samPutInt(std::string &out, int64_t v)
{
    char tmp[24];
    if (v < 0) { out.push_back('-'); v = -v; }
    out.append(tmp, (size_t)(putUint(tmp, (uint64_t)v) - tmp));
}

// NM and MD of a placed read from its list, ungapped or gapped (real_hip_mismatches* / real_hip_mismatches_gapped): `span` text
// positions, `inserted` read bases beside them.  MD: the decimal run of matches, then the text's letter there, alternating, a
// number at either end; a run of deleted entries is ^ and their letters, and a mismatch directly behind it follows a 0.
inline void appendNmMd(std::string &out, const real_hip_mismatch *mm, uint64_t n_mm, uint64_t span, unsigned inserted)
{
    out += "\tNM:i:"; samPutInt(out, (int64_t)(n_mm + inserted));
    out += "\tMD:Z:";
    uint64_t last = 0;
    bool in_deletion = false;
    for (uint64_t k = 0; k < n_mm; ++k) {
        const bool deleted = mm[k].base == REAL_HIP_MISMATCH_DELETED;
        if (!(deleted && in_deletion && mm[k].off == last)) {
            samPutInt(out, (int64_t)(mm[k].off - last));
            if (deleted) out.push_back('^');
        }
        out.push_back("ACGTN"[mm[k].ref < 4 ? mm[k].ref : 4]);
        last = (uint64_t)mm[k].off + 1;
        in_deletion = deleted;
    }
    samPutInt(out, (int64_t)(span - last));
}

// One line.  mate: null for single-end reads; with a mate the line carries the pair flags (which: 64 mate 1, 128 mate 2), RNEXT
// / PNEXT and TLEN, and a trailing /1 or /2 of the read id is dropped.  mm[0 .. n_mm): the placed read's mismatch list.
inline void appendSam(std::string &out, const ReadView &r, const SamRefs &R, const SamPlace &self, const SamPlace *mate, unsigned which, int64_t tlen,
                      const real_hip_mismatch *mm, uint64_t n_mm, bool scores)
{
    const uint64_t patl = r.patl;
    if (out.capacity() < out.size() + r.idlen + 2 * patl + 256) out.reserve(std::max(out.capacity() * 2, out.size() + r.idlen + 2 * patl + 256));
    // QNAME: the id up to the first blank or tab
    size_t ql = 0;
    while (ql < r.idlen && r.id[ql] != ' ' && r.id[ql] != '\t' && r.id[ql] != '\r') ++ql;
    if (mate && ql >= 2 && r.id[ql - 2] == '/' && (r.id[ql - 1] == '1' || r.id[ql - 1] == '2')) ql -= 2;
    out.append(r.id, ql);
    unsigned flag = self.placed ? (self.inverted ? 16u : 0u) : 4u;
    if (self.duplicate) flag |= 1024u;
    if (mate) flag |= 1u | which | (self.paired || self.proper ? 2u : 0u) | (mate->placed ? (mate->inverted ? 32u : 0u) : 8u);
    out.push_back('\t'); samPutInt(out, flag); out.push_back('\t');
    // RNAME POS MAPQ CIGAR: an unplaced mate of a placed one sits where its mate does
    const SamPlace *at = self.placed ? &self : (mate && mate->placed ? mate : nullptr);
    const uint64_t pos1 = at ? at->pos - R.starts[at->file][at->frag] + 1 : 0;
    if (at) out += R.names[at->file][at->frag]; else out.push_back('*');
    out.push_back('\t'); samPutInt(out, (int64_t)pos1);
    if (self.placed) {
        out.push_back('\t'); samPutInt(out, (int64_t)self.mapq); out.push_back('\t');
        if (self.gapped) { out += self.cigar; out.push_back('\t'); } else { samPutInt(out, (int64_t)patl); out += "M\t"; }
    } else out += "\t0\t*\t";
    // RNEXT PNEXT TLEN
    if (!mate || !at) out += "*\t0\t";
    else if (self.placed && mate->placed) {
        if (mate->file == self.file && mate->frag == self.frag) out.push_back('='); else out += R.names[mate->file][mate->frag];
        out.push_back('\t'); samPutInt(out, (int64_t)(mate->pos - R.starts[mate->file][mate->frag] + 1)); out.push_back('\t');
    } else { out += "=\t"; samPutInt(out, (int64_t)pos1); out.push_back('\t'); }
    samPutInt(out, tlen); out.push_back('\t');
    // SEQ QUAL: as placed
    const bool inv = self.placed && self.inverted;
    const size_t s0 = out.size();
    out.resize(s0 + patl);
    char *p = &out[s0];
    if (r.text) {
        if (!inv) for (uint64_t i = 0; i < patl; ++i) p[i] = kSeq.fwd[(unsigned char)r.text[i]];
        else for (uint64_t i = 0; i < patl; ++i) p[i] = kSeq.rc[(unsigned char)r.text[patl - 1 - i]];
    } else {
        if (!inv) for (uint64_t i = 0; i < patl; ++i) p[i] = kSeq.map_fwd[r.mapped[i] < 4 ? r.mapped[i] : 4];
        else for (uint64_t i = 0; i < patl; ++i) { const uint8_t c = r.mapped[patl - 1 - i]; p[i] = kSeq.map_rc[c < 4 ? c : 4]; }
    }
    out.push_back('\t');
    if (!r.qual || !patl) out.push_back('*');
    else {
        const size_t q0 = out.size();
        out.resize(q0 + patl);
        char *q = &out[q0];
        for (uint64_t i = 0; i < patl; ++i) q[i] = (char)((uint8_t)(r.qual[inv ? patl - 1 - i : i] - r.qsub) + 33);
    }
    if (self.placed) {
        appendNmMd(out, mm, n_mm, self.gapped ? self.span : patl, self.inserted);
        if (self.gapped) { out += "\tZC:i:"; samPutInt(out, (int64_t)self.cost); }
        if (scores && !self.gapped) { // (the rescue has no score)
            char b[32];
            out += "\tZS:f:";
            out.append(b, (size_t)fastformat::fmt_g6(self.score, b));
        }
    }
    out.push_back('\n');
}

// ---- which lines the pass of genome file fi writes (last: it is the last file's) -------------------------------------------
// single-end: a read placed in fi; in the last pass the reads placed nowhere
inline void appendSamRead(std::string &out, const ReadView &r, const SamRefs &R, const SamPlace &at, unsigned fi, bool last, const real_hip_mismatch *mm,
                          uint64_t n_mm, bool scores)
{
    if (at.placed ? at.file != fi : !last) return;
    appendSam(out, r, R, at, nullptr, 0, 0, mm, n_mm, scores);
}
// a fragment, mate 1 before mate 2: a mate placed in fi; an unplaced mate beside its mate that is; in the last pass the
// fragments with nothing placed.  mm / moff: the lists of the batch, list 2i + m is mate m of fragment i
inline void appendSamFragment(std::string &out, const ReadView r[2], const SamRefs &R, const SamPlace at[2], unsigned fi, bool last,
                              const real_hip_mismatch *mm, const uint64_t *moff, uint64_t i, bool scores)
{
    for (unsigned m = 0; m < 2; ++m) {
        const SamPlace &self = at[m], &mate = at[1 - m];
        const bool write = self.placed ? self.file == fi : (mate.placed ? mate.file == fi : last);
        if (!write) continue;
        const uint64_t j = 2 * i + m;
        appendSam(out, r[m], R, self, &mate, m ? 128u : 64u, samTlen(self, mate, r[m].patl, r[1 - m].patl), mm + moff[j], moff[j + 1] - moff[j], scores);
    }
}
// -sam_gapped 1: the fragment whose gap record `g` is Unique, in the pass of the record's file (the anchor's: the rescue places
// the other mate beside it).  Both mates have lines, mate 1 first: the anchor's as before but for its mate fields (FLAG without
// 8, with 32 if the rescued mate is inverted; RNEXT / PNEXT; TLEN), the rescued mate's from the record and its gapped list
// gmm[0 .. n_gmm).  The outer distance takes the rescued mate's span on the text for its length; FLAG 2 on both lines iff it
// lies in insert_min .. insert_max.  at[]: the mates as samPlace gives them (the rescued one unplaced); cigar: the record's
// (real_hip_gap_cigar); a fragment of another pass writes nothing.
inline void appendSamRescued(std::string &out, const ReadView r[2], const SamRefs &R, const SamPlace at[2], const real_hip_gap_place &g, const char *cigar, unsigned fi,
                             uint64_t insert_min, uint64_t insert_max, const real_hip_mismatch *mm, const uint64_t *moff, uint64_t i,
                             const real_hip_mismatch *gmm, uint64_t n_gmm, bool scores)
{
    if (g.fileid != fi) return;
    const unsigned t = REAL_HIP_GAP_TARGET(g.tag);
    SamPlace p[2] = {at[0], at[1]};
    p[t] = samPlaceGapped(g, r[t].patl, cigar);
    p[t].duplicate = at[t].duplicate;
    const uint64_t span[2] = {t == 0 ? p[0].span : r[0].patl, t == 1 ? p[1].span : r[1].patl};
    const int64_t outer = samOuter(p[0], p[1], span[0], span[1]);
    p[0].proper = p[1].proper = outer >= (int64_t)insert_min && outer <= (int64_t)insert_max;
    for (unsigned m = 0; m < 2; ++m) {
        const uint64_t j = 2 * i + m;
        const bool target = m == t;
        appendSam(out, r[m], R, p[m], &p[1 - m], m ? 128u : 64u, p[m].inverted ? -outer : outer, target ? gmm : mm + moff[j], target ? n_gmm : moff[j + 1] - moff[j],
                  scores);
    }
}
