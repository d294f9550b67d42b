// Lines.hpp -- the 11-column output lines of `real` (printMatchUnlocked, matchUniqueImplementation.cpp:252-321):
// a read as the formatter needs it (ReadView), where reads come from (ReadSource: a text chunk of the read file with
// its spans, or a block of the host reader), one line for a read and a placement (appendLine), and the lines of a
// block of reads formatted by all host threads and written in read order (formatAndWrite).  formatAndWrite accounts
// its time, so the run's clock and stage timers are here too (now_s, Timers), and Chunk, the text a ReadSource reads.
// Beside this file: RawChunker.hpp cuts the read file into Chunks; Sam.hpp and Vcf.hpp hold the lines of -sam and -vcf;
// real.cpp holds the passes of a run and everything that calls the library.
// Host code only: nothing here calls into the library.
#pragma once
#include <omp.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "FastFormat.hpp"
#include "ReadReader.hpp"

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// where the wall time of a run went, from the construction on; finish() prints it as one "timing:" line on stderr
// (bench_support/cli_midsize.py reads it)
struct Timers {
    const double begin = now_s();
    double genome = 0, index = 0, read = 0, parse = 0, match = 0, format = 0, write = 0;
    uint64_t out_bytes = 0;
    void finish(uint64_t reads, uint64_t lines) const
    {
        fprintf(stderr, "timing: genome_load_s=%.3f index_s=%.3f read_file_s=%.3f parse_s=%.3f match_s=%.3f format_s=%.3f write_s=%.3f total_s=%.3f reads=%llu lines=%llu out_bytes=%llu\n",
                genome, index, read, parse, match, format, write, now_s() - begin, (unsigned long long)reads, (unsigned long long)lines, (unsigned long long)out_bytes);
    }
};

// ---- a read for output ------------------------------------------------------------------------------------------
// A chunk of whole records of the read file, as text (RawChunker.hpp), and what the device parser found in it:
// per read where its id starts and how long it is, and the running sum of the sequence lengths.
struct Chunk {
    char *text = nullptr;
    size_t cap = 0, size = 0;
    uint64_t file_offset = 0; // of text[0]
};
struct Spans {
    std::vector<uint32_t> id_start, id_len;
    std::vector<uint64_t> off; // n+1
};

// the sequence either as the characters of the read file (text) or as mapped symbols (mapped): the other one is null.
// qual: the quality of base i is (uint8_t)(qual[i] - qsub) -- the characters of the read file less the quality offset, or
// the host reader's values less 0; null for FASTA, and for a source that was not asked for the qualities (withQuality)
struct ReadView {
    const char *id;
    size_t idlen;
    const char *text;
    const uint8_t *mapped;
    uint64_t patl;
    const uint8_t *qual;
    uint8_t qsub;
};

class ReadSource {
public:
    ReadSource(const Chunk &c, const Spans &s)
        : text_(c.text), text_end_(c.text + c.size), id_start_(s.id_start.data()), id_len_(s.id_len.data()), off_(s.off.data()), n_(s.id_start.size()) {}
    explicit ReadSource(const ReadBlock &b) : blk_(&b) {} // (follows the block: what the reader fills in next is seen)
    // the same reads with their qualities in the views (the SAM lines): of a FASTQ file read with quality offset qoff
    ReadSource withQuality(bool fastq, int qoff) const
    {
        ReadSource r = *this;
        r.qoff_ = fastq ? qoff : -1;
        return r;
    }
    uint64_t size() const { return blk_ ? blk_->size() : n_; }
    ReadView operator[](uint64_t i) const
    {
        ReadView v;
        if (blk_) {
            const uint64_t lo = blk_->offsets[i];
            v.id = blk_->ids[i].data(); v.idlen = blk_->ids[i].size();
            v.text = nullptr; v.mapped = &blk_->bases[lo];
            v.patl = blk_->offsets[i + 1] - lo;
            v.qual = qoff_ >= 0 ? &blk_->qual[lo] : nullptr; v.qsub = 0;
        } else {
            // the id is everything behind the marker up to the newline (a '\r' in front of it included, as the
            // reference's reader keeps it); the sequence is the next line
            v.id = text_ + id_start_[i]; v.idlen = id_len_[i];
            if (v.id[v.idlen] == '\r') v.idlen++;
            v.text = v.id + v.idlen + 1; v.mapped = nullptr;
            v.patl = off_[i + 1] - off_[i];
            v.qual = nullptr; v.qsub = 0;
            if (qoff_ >= 0) { // one line per field: behind the sequence line comes the '+' line, then the qualities
                const char *q = (const char *)memchr(v.text + v.patl, '\n', (size_t)(text_end_ - (v.text + v.patl)));
                if (q) q = (const char *)memchr(q + 1, '\n', (size_t)(text_end_ - (q + 1)));
                if (q && q + 1 + v.patl <= text_end_) { v.qual = (const uint8_t *)(q + 1); v.qsub = (uint8_t)qoff_; }
            }
        }
        return v;
    }
private:
    const char *text_ = nullptr, *text_end_ = nullptr; // a chunk and its n_ spans (as they are when the source is made), or
    const uint32_t *id_start_ = nullptr, *id_len_ = nullptr;
    const uint64_t *off_ = nullptr;
    uint64_t n_ = 0;
    const ReadBlock *blk_ = nullptr; // a block
    int qoff_ = -1;                  // >= 0: the views carry the qualities
};

// where a read lies: pos1 is the 1-based position in the fragment; the score is printed only where scores are on
struct Placement {
    float score;
    bool inverted;
    const std::string &fragname;
    uint64_t pos1;
    unsigned errors;
};

// ---- one line ---------------------------------------------------------------------------------------------------
// id \t sequence as matched \t score|"" \t 1 \t a \t patl \t +|- \t fragment name \t 1-based position \t "" \t errors \n
// Written straight into the thread's buffer: table lookups for the sequence, hand-rolled decimal numbers, and the score by
// fastformat::fmt_g6 -- the digits of printf's %g, which is what operator<<(float) prints, from integer arithmetic.
struct SeqTables {
    char fwd[256], rc[256], map_fwd[5], map_rc[5];
    SeqTables()
    {
        for (int c = 0; c < 256; ++c) { fwd[c] = 'N'; rc[c] = 'N'; }   // anything but ACGT (lowercase too) maps to 4 and prints as N
        fwd['A'] = 'A'; fwd['C'] = 'C'; fwd['G'] = 'G'; fwd['T'] = 'T';
        rc['A'] = 'T'; rc['C'] = 'G'; rc['G'] = 'C'; rc['T'] = 'A';
        memcpy(map_fwd, "ACGTN", 5); memcpy(map_rc, "TGCAN", 5);       // remapChar, acgtnMap.hpp:24-35; transposed: 3 - c
    }
};
static const SeqTables kSeq;

inline char *putUint(char *p, uint64_t v)
{
    char tmp[24];
    int n = 0;
    do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (n) *p++ = tmp[--n];
    return p;
}
// (always inlined, and ReadSource holds plain pointers: through the Spans' vectors, which any stored character may alias, the mid-size run formats in 0.08 s, not 0.06)
__attribute__((always_inline)) inline void appendLine(std::string &out, const ReadView &r, bool scores, const Placement &at)
{
    const size_t start = out.size(), room = start + r.idlen + r.patl + at.fragname.size() + 112;
    const uint64_t patl = r.patl;
    if (out.capacity() < room) out.reserve(std::max(out.capacity() * 2, room));
    out.resize(room);
    char *p = &out[start], *p0 = p;
    memcpy(p, r.id, r.idlen); p += r.idlen;
    *p++ = '\t';
    if (r.text) {
        if (!at.inverted) for (uint64_t i = 0; i < patl; ++i) p[i] = kSeq.fwd[(unsigned char)r.text[i]];
        else for (uint64_t i = 0; i < patl; ++i) p[i] = kSeq.rc[(unsigned char)r.text[patl - 1 - i]];
    } else {
        if (!at.inverted) for (uint64_t i = 0; i < patl; ++i) p[i] = kSeq.map_fwd[r.mapped[i] < 4 ? r.mapped[i] : 4];
        else for (uint64_t i = 0; i < patl; ++i) { const uint8_t c = r.mapped[patl - 1 - i]; p[i] = kSeq.map_rc[c < 4 ? c : 4]; }
    }
    p += patl;
    *p++ = '\t';
    if (scores) p += fastformat::fmt_g6(at.score, p); // operator<<(float): %g, six significant digits
    memcpy(p, "\t1\ta\t", 5); p += 5;
    p = putUint(p, patl);
    *p++ = '\t'; *p++ = at.inverted ? '-' : '+'; *p++ = '\t';
    memcpy(p, at.fragname.data(), at.fragname.size()); p += at.fragname.size();
    *p++ = '\t';
    p = putUint(p, at.pos1);
    *p++ = '\t'; *p++ = '\t';
    p = putUint(p, at.errors);
    *p++ = '\n';
    out.resize(start + (size_t)(p - p0));
}

struct Record { unsigned st, frag, errors, file; uint64_t pos; };
inline Record unpack(uint64_t rec)
{
    Record r;
    r.st = (unsigned)(rec >> 61); r.frag = (rec >> 45) & 0xffff; r.errors = (rec >> 41) & 15; r.file = (rec >> 35) & 63; r.pos = rec & ((1ull << 35) - 1);
    return r;
}

// ---- the lines of a block ---------------------------------------------------------------------------------------
// The lines of reads [0, n) of one block, formatted by all host threads (each a contiguous range of reads into its
// own buffer) and written in read order with one large write per buffer.  line(i, out) appends read i's line(s).
// (128 bytes apart, so that no two strings share a cache line: the threads update their string's length line by line.
// By padding and not by alignas: operator new of C++14 does not align a vector's storage beyond max_align_t.)
struct LineBuf { std::string s; char pad[128 - sizeof(std::string)]; };

template <class LineFn>
void formatAndWrite(uint64_t n, FILE *out, Timers &T, LineFn line)
{
    const int nt = std::max(1, omp_get_max_threads());
    static std::vector<LineBuf> buf; // (kept across calls: the pages of a buffer are touched once, not once per block)
    if ((int)buf.size() < nt) buf = std::vector<LineBuf>((size_t)nt);
    const double t0 = now_s();
#pragma omp parallel num_threads(nt)
    {
        const int t = omp_get_thread_num();
        const uint64_t lo = n * (uint64_t)t / nt, hi = n * (uint64_t)(t + 1) / nt;
        std::string b;
        b.swap(buf[(size_t)t].s); // (worked on as a local: its length and pointer live in registers / this thread's stack)
        b.clear();
        for (uint64_t i = lo; i < hi; ++i) line(i, b);
        b.swap(buf[(size_t)t].s);
    }
    const double t1 = now_s();
    for (int t = 0; t < nt; ++t) {
        const std::string &b = buf[(size_t)t].s;
        if (!b.empty() && fwrite(b.data(), 1, b.size(), out) != b.size()) throw std::runtime_error("write to the output file failed");
        T.out_bytes += b.size();
    }
    T.format += t1 - t0; T.write += now_s() - t1;
}
