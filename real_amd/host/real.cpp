// real.cpp -- the `real` command line on top of the C ABI (include/real_hip.h).
//
// Host side of the drop-in: keeps the reference's CLI surface (real.cpp:357-375 main,
// cpuMain :295-354), RealOptions, FASTA/FASTQ input and the 11-column TSV output
// (printMatchUnlocked, matchUniqueImplementation.cpp:252-321; matchAll inline :481-518), and
// replaces the OpenMP per-read loops of EnumerateUniqueMatches::doMatching
// (matchUniqueImplementation.cpp:1082-1489) / EnumerateAllMatches::doMatching
// (matchAllImplementation.cpp:359-538) by calls into libreal_hip.so.  Loop structure as in the
// reference: genome files -> index blocks -> all reads re-streamed per block -> output.
//
// The read file travels as text: chunks of whole records are read into pinned buffers by a prefetch
// thread, parsed and matched on the device(s) (real_hip_parse_reads + real_hip_match_unique), and in the
// output pass parsed again for the id / sequence spans, from which the host formats the lines with all
// its cores and writes them with large sequential writes.  A file (or a later part of one) that is not in
// one-line-per-field form is read by the host reader from that record on.
//
// Here: what the four drivers share and the drivers.  Shared: an ABI struct made and a stage's statistics read one way
// (sized, readStats), genomePass, the read file streamed (streamReads; restreamReads for a later pass, which must find the
// reads of the first) and the two mate files likewise (streamMates, restreamMates), OutFile, the lists that grow
// (listGrowing, Lists::fill), one gap leg, gap line and empty gap record, and the marks behind "All done.".  Each driver reads top
// to bottom as the run goes: match, "All done.", marks, output, the passes behind the output.  Each formats through one lambda --
// read i of a ReadSource and a Placement, whatever parsed the read (Lines.hpp: all about the lines; RawChunker.hpp: the read
// file as text chunks).
//
// Deliberate differences from reference quirks (SURVEY 8a "quirks"): matchAll handles FASTQ input
// (quirk 1) and writes every line (quirk 2); the exit status is non-zero on errors (quirk 6).
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "GenomeText.hpp"
#include "HostIndex.hpp"
#include "Lines.hpp"
#include "RawChunker.hpp"
#include "ReadReader.hpp"
#include "RealOptions.hpp"
#include "Sam.hpp"
#include "Vcf.hpp"
#include "real_hip.h"

namespace {

struct Ctx {
    real_hip_ctx *h = nullptr;
    ~Ctx() { if (h) real_hip_destroy(h); }
};
typedef std::vector<std::unique_ptr<Ctx>> CtxVec;

void check(real_hip_ctx *h, int rc, const char *what)
{
    if (rc == REAL_HIP_OK) return;
    std::string msg = std::string(what) + ": " + real_hip_strerror(rc);
    if (h && *real_hip_last_error(h)) msg += std::string(" (") + real_hip_last_error(h) + ")";
    if (rc == REAL_HIP_E_NOMEM) throw std::bad_alloc(); // "Insufficient memory", matchUniqueImplementation.cpp:1215-1219
    throw std::runtime_error(msg);
}

// An ABI struct as the library takes it: every field zero, which each of them reads as "absent", and struct_size set.
template <class S>
S sized()
{
    S s = S();
    s.struct_size = sizeof s;
    return s;
}
// the statistics of a stage: get(h, &st, reset) into such a struct
template <class S>
S readStats(real_hip_ctx *h, int (*get)(real_hip_ctx *, S *, int), int reset, const char *what)
{
    S st = sized<S>();
    check(h, get(h, &st, reset), what);
    return st;
}

// the contexts of the run: one per device of -gpus, or `gpus` of them (the pileup pass: one, on -device)
CtxVec makeContexts(const RealOptions &o, int gpus = 0)
{
    if (!gpus) gpus = o.gpus;
    real_hip_params p = sized<real_hip_params>();
    p.seedl = o.seedl; p.seedkmax = o.seedkmax; p.totalkmax = o.totalkmax; p.scores = o.scores;
    p.prefix_bits = o.prefix_bits; p.table_kind = o.table_kind; p.filter_mult = o.filter_mult;
    real_hip_scoring_table(o.similarity, o.gc, o.trans, o.err, o.gcmut_bias, p.LL); // Scoring(opts...) :1115
    CtxVec v;
    for (int g = 0; g < gpus; ++g) {
        p.device = o.gpus_share_device ? o.device : o.device + g;
        std::unique_ptr<Ctx> c(new Ctx);
        check(nullptr, real_hip_create(&c->h, &p), "real_hip_create (is an MI355X visible? there is no CPU fallback)");
        v.push_back(std::move(c));
    }
    return v;
}

// run f(g) for g in [0, n) on one host thread per context; the first exception is rethrown
template <class F>
void onEach(size_t n, F f)
{
    if (n == 1) { f((size_t)0); return; }
    std::vector<std::thread> th;
    std::vector<std::string> errs(n);
    std::vector<int> nomem(n, 0);
    for (size_t g = 0; g < n; ++g)
        th.emplace_back([&, g]() {
            try { f(g); } catch (const std::bad_alloc &) { nomem[g] = 1; } catch (const std::exception &e) { errs[g] = e.what(); if (errs[g].empty()) errs[g] = "error"; }
        });
    for (auto &t : th) t.join();
    for (size_t g = 0; g < n; ++g) if (nomem[g]) throw std::bad_alloc();
    for (auto &e : errs) if (!e.empty()) throw std::runtime_error(e);
}

// positions per index block from the HBM budget: the tables of a block plus the transients of its build
// (the device-side analogue of matchUniqueImplementation.cpp:1221-1244)
uint64_t blockEntries(const RealOptions &o, real_hip_ctx *h, uint64_t windows)
{
    if (o.block_entries) return o.block_entries;
    uint64_t fr = 0, tot = 0;
    check(h, real_hip_device_memory(h, &fr, &tot), "real_hip_device_memory");
    const double budget = o.fracmem * (double)fr - 6.0 * 4.0 * (double)(1ull << 30) - 2e9;
    uint64_t cap = budget > 0 ? (uint64_t)(budget / 64.0) : (1u << 20);
    if (cap < (1u << 20)) cap = 1u << 20;
    return windows < cap ? windows : cap;
}

struct Ranges { std::vector<std::vector<std::string>> names; std::vector<std::vector<uint64_t>> starts; };

// the quality offset of a FASTQ read file: -Q, or detected from the file (0 for FASTA)
int qualityOffset(const RealOptions &o, bool fastq, const std::string &filename)
{
    if (!fastq) return 0;
    const int qoff = o.qualityOffset ? (int)o.qualityOffset : ReadReader::getOffset(filename);
    if (!qoff) throw std::runtime_error("Unable to automatically detect FastQ quality format."); // :1112
    return qoff;
}

// the genome files of -t; too_many: the error for more than 64 of them where the records hold a file id of 6 bits
std::vector<std::string> genomeFiles(const RealOptions &o, const char *too_many)
{
    std::vector<std::string> files;
    getFileList(o.textfilename, files);
    if (files.empty()) throw std::runtime_error("no .fa text file found at " + o.textfilename);
    if (too_many && files.size() > 64) throw std::runtime_error(too_many);
    return files;
}

// An output file behind a buffer of 8 MiB ("-": standard output; the -unpaired file is always a file).  close() is the
// regular end.  The destructor is the way out through an exception: what the buffer holds is written while the buffer
// still exists, so lines formatted before an error reach the file.  (Standard output keeps pointing at the buffer, empty
// from then on: nothing is written to it behind the drivers.)
class OutFile {
public:
    // flag: the file of another flag than -o (never standard output), named in the errors
    explicit OutFile(const std::string &filename, bool unpaired = false, const char *flag = nullptr) : flag_(unpaired ? "-unpaired" : flag), buf_((size_t)8 << 20)
    {
        f_ = (!flag_ && filename == "-") ? stdout : fopen(filename.c_str(), "wb");
        if (!f_) throw std::runtime_error((flag_ ? std::string("cannot open the ") + flag_ + " file " : std::string("cannot open output file ")) + filename);
        setvbuf(f_, buf_.data(), _IOFBF, buf_.size());
    }
    ~OutFile() { if (f_ == stdout) fflush(f_); else if (f_) fclose(f_); }
    OutFile(const OutFile &) = delete;
    OutFile &operator=(const OutFile &) = delete;
    FILE *file() const { return f_; }
    void close()
    {
        if (fflush(f_) != 0) throw std::runtime_error(flag_ ? std::string("write to the ") + flag_ + " file failed" : std::string("write to the output file failed"));
        if (f_ != stdout) fclose(f_);
        f_ = nullptr;
    }
private:
    const char *flag_;
    std::vector<char> buf_;
    FILE *f_;
};

// text + one index block on every device
struct Resident {
    GenomeText G;
    std::vector<uint32_t> wpos; // host index only
    std::vector<uint64_t> text2bit, wildbits;
};

void setText(const RealOptions &o, CtxVec &ctx, Resident &R, unsigned fi)
{
    if (o.host_index) { R.G.pack(R.text2bit, R.wildbits); enumerateWindows(R.G.sym, o.seedl, R.wpos); }
    onEach(ctx.size(), [&](size_t g) {
        real_hip_ctx *h = ctx[g]->h;
        if (o.host_index)
            check(h, real_hip_set_text(h, fi, R.text2bit.data(), R.wildbits.data(), R.G.sym.size(), R.G.frag_start.data(),
                                       (uint32_t)R.G.frag_names.size()), "real_hip_set_text");
        else
            check(h, real_hip_set_text_symbols(h, fi, R.G.sym.data(), R.G.sym.size(), 0, R.G.frag_start.data(),
                                               (uint32_t)R.G.frag_names.size()), "real_hip_set_text_symbols");
    });
}

// returns entries of the block, sets have_next
uint64_t nextBlock(const RealOptions &o, CtxVec &ctx, Resident &R, uint64_t first, uint64_t n_list, bool &have_next)
{
    uint64_t n = 0;
    if (o.host_index) {
        HostIndexBlock B;
        buildHostIndexBlock(R.G.sym, R.wpos, o.seedl, first, n_list, (int)o.sort_threads, B);
        const void *sg[6]; const uint32_t *ps[6];
        for (int k = 0; k < 6; ++k) { sg[k] = B.sign_ptr(k); ps[k] = B.pos[k].data(); }
        onEach(ctx.size(), [&](size_t g) { check(ctx[g]->h, real_hip_set_index_block(ctx[g]->h, B.n, sg, ps), "real_hip_set_index_block"); });
        n = B.n; have_next = B.have_next;
    } else {
        std::vector<uint64_t> ns(ctx.size(), 0);
        std::vector<int> hn(ctx.size(), 0);
        onEach(ctx.size(), [&](size_t g) {
            check(ctx[g]->h, real_hip_build_index_block(ctx[g]->h, first, n_list, &ns[g], &hn[g]), "real_hip_build_index_block");
        });
        n = ns[0]; have_next = hn[0] != 0;
    }
    std::cerr << "Obtained " << n << " fragments of size " << o.seedl << std::endl; // ListSetBlockReader.hpp:36
    return n;
}

// ---- one genome file -----------------------------------------------------------------------------------
// Genome file fi announced (kSayLast: with the note on the last one), loaded, its text put on every device and its index
// blocks made resident one after the other: onBlock(R) runs with each of them.  kOneBlock: paired-end reads, whose pairs
// across two blocks would be lost -- a file that needs a second block is refused.  RS, where given, collects the
// fragments of all files for the output behind the last one.
enum { kSayLast = 1, kOneBlock = 2 };
template <class OnBlock>
void genomePass(const RealOptions &o, CtxVec &ctx, const std::vector<std::string> &files, unsigned fi, int how, Timers &T, Ranges *RS, OnBlock onBlock)
{
    std::cerr << "Processing file " << files[fi] << (((how & kSayLast) && fi + 1 == files.size()) ? " (last processed file)" : "") << std::endl;
    Resident R;
    double t0 = now_s();
    R.G.load(files[fi]);
    T.genome += now_s() - t0;
    if (RS) { RS->names.push_back(R.G.frag_names); RS->starts.push_back(R.G.frag_start); }
    t0 = now_s();
    setText(o, ctx, R, fi);
    T.index += now_s() - t0;
    const uint64_t n_list = blockEntries(o, ctx[0]->h, R.G.sym.size() ? R.G.sym.size() : 1);
    uint64_t first = 0;
    bool have_next = true;
    while (have_next) {
        t0 = now_s();
        const uint64_t n = nextBlock(o, ctx, R, first, n_list, have_next);
        T.index += now_s() - t0;
        if ((how & kOneBlock) && have_next)
            throw std::runtime_error("paired-end reads: " + files[fi] + " needs more than one index block (pairs across blocks would be lost); "
                                     "raise -f / -block or split the file");
        if (!n) break;
        first += n;
        onBlock(R);
    }
}

real_hip_batch makeBatch(const ReadBlock &b)
{
    real_hip_batch rb = sized<real_hip_batch>();
    rb.on_device = 0; rb.n_reads = b.size();
    rb.bases = b.bases.data(); rb.qual = b.qual.data(); rb.offsets = b.offsets.data();
    return rb;
}
real_hip_batch makeBatch(const real_hip_parsed &p)
{
    real_hip_batch rb = sized<real_hip_batch>();
    rb.on_device = 2; rb.n_reads = p.n_reads;
    rb.bases = p.bases; rb.qual = p.qual; rb.offsets = p.offsets; rb.max_patl = p.max_patl;
    return rb;
}

// One round's share of one context: its reads as a batch for the matcher and, in a pass that wants the ids, as the
// source of the formatter.
struct ReadItem {
    uint64_t first_id;
    real_hip_batch batch;
    ReadSource src;
};

// what the device parser found in a chunk, for the formatter
void downloadSpans(real_hip_ctx *h, const real_hip_parsed &p, Spans &sp, Timers &T)
{
    const uint64_t n = p.n_reads;
    sp.id_start.resize(n); sp.id_len.resize(n); sp.off.resize(n + 1);
    if (!n) return;
    const double t0 = now_s();
    check(h, real_hip_download(h, p.id_start, sp.id_start.data(), n * 4), "real_hip_download");
    check(h, real_hip_download(h, p.id_len, sp.id_len.data(), n * 4), "real_hip_download");
    check(h, real_hip_download(h, p.offsets, sp.off.data(), (n + 1) * 8), "real_hip_download");
    T.parse += now_s() - t0;
}

// One pass over the read file.  Rounds of up to one chunk per context: parsed on the devices, then onRound(items) sees
// them (in file order, item g on context g).  From the first chunk a device parser refuses (text not in one-line-per-
// field form) the host reader takes over at that record: onRound sees rounds of host-parsed blocks.  A file that is
// refused from its first chunk on -- or -gpuparse 0 -- is read by the host reader alone.
// Returns the number of reads seen.
template <class OnRound>
uint64_t streamReads(const RealOptions &o, CtxVec &ctx, int qoff, bool want_ids, Timers &T, OnRound onRound)
{
    uint64_t next_id = 0, takeover_at = 0;
    bool host = !o.gpuparse;
    std::vector<ReadItem> items;
    std::vector<Spans> spans(ctx.size());
    if (!host) {
        RawChunker rc(o.patternfilename, o.fastq, o.chunk_bytes, 2 * ctx.size(), real_hip_host_alloc, real_hip_host_free); // (pinned: the chunks cross PCIe by DMA)
        while (!host) {
            std::vector<Chunk> ch;
            for (size_t g = 0; g < ctx.size(); ++g) {
                Chunk c;
                if (!rc.next(c, T.read)) break;
                ch.push_back(c);
            }
            if (ch.empty()) break;
            std::vector<real_hip_parsed> pr(ch.size());
            std::vector<int> prc(ch.size(), 0);
            const double t0 = now_s();
            onEach(ch.size(), [&](size_t g) {
                prc[g] = real_hip_parse_reads(ctx[g]->h, ch[g].text, ch[g].size, 0, o.fastq ? 1 : 0, qoff, &pr[g]);
            });
            T.parse += now_s() - t0;
            size_t good = 0;
            for (; good < ch.size(); ++good) {
                if (prc[good] == REAL_HIP_E_UNSUPPORTED) break;
                check(ctx[good]->h, prc[good], "real_hip_parse_reads");
            }
            if (good < ch.size()) { host = true; takeover_at = ch[good].file_offset; }
            ch.resize(good); pr.resize(good);
            if (good) {
                items.clear();
                for (size_t g = 0; g < good; ++g) {
                    if (want_ids) downloadSpans(ctx[g]->h, pr[g], spans[g], T);
                    items.push_back(ReadItem{next_id, makeBatch(pr[g]), ReadSource(ch[g], spans[g])});
                    next_id += pr[g].n_reads;
                }
                onRound(items);
            }
            for (auto &c : ch) rc.release(c);
        }
        if (host) std::cerr << "read file leaves the one-line-per-field form at byte " << takeover_at << ": the host reader takes over from there" << std::endl;
    }
    if (host) {
        ReadReader rr(o.patternfilename, o.fastq, qoff, takeover_at, next_id); // the whole read set is re-streamed per block, :1260
        std::vector<ReadBlock> blk(ctx.size());
        while (true) {
            size_t used = 0;
            const double t0 = now_s();
            for (; used < ctx.size(); ++used)
                if (!rr.fillBlock(blk[used], o.batch_reads, want_ids)) break;
            T.parse += now_s() - t0;
            if (!used) break;
            items.clear();
            for (size_t g = 0; g < used; ++g) items.push_back(ReadItem{blk[g].first_id, makeBatch(blk[g]), ReadSource(blk[g])});
            onRound(items);
            for (size_t g = 0; g < used; ++g) next_id += blk[g].size();
        }
    }
    return next_id;
}

// A later pass over the read file, which must hold the numpat reads the first pass counted: onItem(g, item) runs with every
// item that has reads, the items of a round each on a host thread of its own (item g belongs to context g; one context: one
// item, on the caller's thread).  round_s, where given, receives the wall time of the rounds.
const char *const kReadFileChanged = "the read file changed between two passes";
template <class OnItem>
void restreamReads(const RealOptions &o, CtxVec &ctx, int qoff, bool want_ids, Timers &T, uint64_t numpat, double *round_s, OnItem onItem)
{
    const uint64_t seen = streamReads(o, ctx, qoff, want_ids, T, [&](const std::vector<ReadItem> &items) {
        const double tm = now_s();
        onEach(items.size(), [&](size_t g) {
            const ReadItem &it = items[g];
            if (!it.batch.n_reads) return;
            if (it.first_id + it.batch.n_reads > numpat) throw std::runtime_error(kReadFileChanged);
            onItem(g, it);
        });
        if (round_s) *round_s += now_s() - tm;
    });
    if (seen != numpat) throw std::runtime_error(kReadFileChanged);
}

// list(h, in..., hits, room, &n, offsets) lists into hits and answers REAL_HIP_E_OVERFLOW with the number it has to list:
// retried once with room for them.  Returns the number listed.
template <class Hit, class List, class... In>
uint64_t listGrowing(real_hip_ctx *h, const char *what, std::vector<Hit> &hits, uint64_t *offsets, List list, In... in)
{
    uint64_t n = 0;
    int rc = list(h, in..., hits.data(), hits.size(), &n, offsets);
    if (rc == REAL_HIP_E_OVERFLOW) { // retry with the size the library reports
        hits.resize(n + 16);
        rc = list(h, in..., hits.data(), hits.size(), &n, offsets);
    }
    check(h, rc, what);
    return n;
}

// ---- -pileup / -pileup_depth: the final placements piled up over every genome file -----------------------------
// Runs behind the output pass, when the matching contexts are gone: one fresh context on -device takes the genome files in
// order -- the text alone, no index -- and for each of them real_hip_pileup_begin, the reads once more through
// addAll(ctx), which hands every batch with its final records to real_hip_pileup_add / _add_pairs, and
// real_hip_pileup_finish.  The sites and the depth runs of all files go to the two files, a summary line per file to
// standard error.
const uint64_t kDepthWindow = (uint64_t)64 << 20; // positions of depth[] fetched at a time

void writeSites(real_hip_ctx *h, uint64_t n_sites, const GenomeText &G, FILE *f)
{
    std::vector<real_hip_pileup_site> sites(n_sites);
    uint64_t n = 0;
    check(h, real_hip_pileup_sites(h, sites.data(), sites.size(), &n, 0), "real_hip_pileup_sites");
    size_t fr = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const real_hip_pileup_site &S = sites[k];
        while (fr + 1 < G.frag_names.size() && G.frag_start[fr + 1] <= S.pos) ++fr; // (ascending positions)
        fprintf(f, "%s\t%llu\t%c\t%u\t%u\t%u\t%u\t%u\n", G.frag_names[fr].c_str(), (unsigned long long)(S.pos - G.frag_start[fr] + 1), "ACGT"[S.ref & 3u],
                S.depth, S.alt[0], S.alt[1], S.alt[2], S.alt[3]);
    }
}

// maximal runs of equal non-zero depth that do not cross a fragment boundary, from windows of depth[]
void writeDepthRuns(real_hip_ctx *h, const GenomeText &G, FILE *f)
{
    const uint64_t n = G.sym.size();
    std::vector<uint32_t> win((size_t)std::min<uint64_t>(n, kDepthWindow));
    size_t fr = 0;
    uint64_t run_start = 0;
    uint32_t run_depth = 0;
    auto flush = [&](uint64_t end) {
        if (run_depth) fprintf(f, "%s\t%llu\t%llu\t%u\n", G.frag_names[fr].c_str(), (unsigned long long)(run_start - G.frag_start[fr]),
                               (unsigned long long)(end - G.frag_start[fr]), run_depth);
    };
    for (uint64_t first = 0; first < n; first += kDepthWindow) {
        const uint64_t count = std::min<uint64_t>(kDepthWindow, n - first);
        check(h, real_hip_pileup_depth(h, first, count, win.data(), 0), "real_hip_pileup_depth");
        for (uint64_t k = 0; k < count; ++k) {
            const uint64_t x = first + k;
            if (fr + 1 < G.frag_names.size() && x == G.frag_start[fr + 1]) { flush(x); ++fr; run_start = x; run_depth = 0; }
            if (win[k] != run_depth) { flush(x); run_start = x; run_depth = win[k]; }
        }
    }
    flush(n);
}

// What the passes behind the output pass share (-pileup, -sam): one fresh context on -device takes the genome files in order,
// the text alone, and perFile(ctx, fi, G) runs with each of them resident.
template <class PerFile>
void textPass(const RealOptions &o, const std::vector<std::string> &files, Timers &T, PerFile perFile)
{
    double t0 = now_s();
    CtxVec ctx = makeContexts(o, 1);
    real_hip_ctx *h = ctx[0]->h;
    T.index += now_s() - t0; // (the context and the texts: what the matching contexts' index time holds too)
    for (unsigned fi = 0; fi < files.size(); ++fi) {
        GenomeText G;
        t0 = now_s();
        G.load(files[fi]);
        T.genome += now_s() - t0;
        t0 = now_s();
        check(h, real_hip_set_text_symbols(h, fi, G.sym.data(), G.sym.size(), 0, G.frag_start.data(), (uint32_t)G.frag_names.size()), "real_hip_set_text_symbols");
        T.index += now_s() - t0;
        perFile(ctx, fi, G);
    }
}
inline bool passesBehindOutput(const RealOptions &o)
{
    return o.pileup_given || o.pileup_depth_given || o.vcf_given || o.sam_given || o.gapped_given || o.gapped_single_given;
}

// -vcf: the calls of the finished pileup of one genome file (real_hip_call_*) -- the reads once more through
// addAll(ctx, true), which hands every batch with its final records to real_hip_call_add / _add_pairs -- as VCF lines, and a
// summary line to standard error.
// -vcf_indels 1 (real_hip_indel_*): behind the SNP calls, on the same finished pileup, indelAll(ctx, fi) hands the
// reads once more to the gap rescue and every batch's gap records to real_hip_indel_add; the indel calls are merged into the
// file's lines by position, and a second summary line goes to standard error
// -pileup_gapped 1: behind the ungapped evidence, gapAll(ctx, fi, kGapCalls) hands the gap records the pileup pass
// made to real_hip_call_add_gapped
enum GapLeg { kGapPileup, kGapCalls, kGapIndels };
template <class AddAll, class GapAll>
void writeCalls(const RealOptions &o, CtxVec &ctx, unsigned fi, const std::string &file, const std::vector<std::string> &names, const GenomeText &G, FILE *f,
                AddAll addAll, GapAll gapAll)
{
    real_hip_ctx *h = ctx[0]->h;
    check(h, real_hip_call_begin(h), "real_hip_call_begin");
    addAll(ctx, true);
    if (o.pileup_gapped) gapAll(ctx, fi, kGapCalls);
    real_hip_call_params cp = sized<real_hip_call_params>();
    cp.min_call_qual = (uint32_t)o.vcf_minqual; cp.min_depth = (uint32_t)o.vcf_mindepth;
    uint64_t n_calls = 0, n = 0;
    check(h, real_hip_call_finish(h, &cp, &n_calls), "real_hip_call_finish");
    std::vector<real_hip_call> calls(n_calls);
    check(h, real_hip_call_variants(h, calls.data(), calls.size(), &n, 0), "real_hip_call_variants");
    std::vector<real_hip_indel> indels;
    if (o.vcf_indels) {
        check(h, real_hip_indel_begin(h), "real_hip_indel_begin");
        gapAll(ctx, fi, kGapIndels);
        real_hip_indel_params ip = sized<real_hip_indel_params>();
        ip.min_call_qual = (uint32_t)o.vcf_minqual; ip.min_alt = (uint32_t)o.vcf_minalt; ip.min_depth = (uint32_t)o.vcf_mindepth;
        uint64_t n_events = 0, n_indels = 0, ni = 0;
        check(h, real_hip_indel_finish(h, &ip, &n_events, &n_indels), "real_hip_indel_finish");
        indels.resize(n_indels);
        check(h, real_hip_indel_calls(h, indels.data(), indels.size(), &ni, 0), "real_hip_indel_calls");
    }
    writeVcfMerged(f, names, G.frag_start.data(), G.sym.data(), calls.data(), n, indels.data(), indels.size());
    const real_hip_pileup_stats ps = readStats(h, real_hip_pileup_stats_get, 0, "real_hip_pileup_stats_get");
    const real_hip_call_stats st = readStats(h, real_hip_call_stats_get, 1, "real_hip_call_stats_get");
    fprintf(stderr, "calls: file=%s sites=%llu calls=%llu het=%llu hom=%llu site_bases=%llu low_qual=%llu\n", file.c_str(), (unsigned long long)ps.sites,
            (unsigned long long)st.calls, (unsigned long long)st.het, (unsigned long long)st.hom, (unsigned long long)st.site_bases, (unsigned long long)st.low_qual);
    if (o.vcf_indels) {
        const real_hip_indel_stats is = readStats(h, real_hip_indel_stats_get, 1, "real_hip_indel_stats_get");
        fprintf(stderr, "indels: file=%s events=%llu distinct=%llu calls=%llu het=%llu hom=%llu deletions=%llu insertions=%llu shifted=%llu low_qual=%llu\n",
                file.c_str(), (unsigned long long)is.events, (unsigned long long)is.distinct, (unsigned long long)is.calls, (unsigned long long)is.het,
                (unsigned long long)is.hom, (unsigned long long)is.deletions, (unsigned long long)is.insertions, (unsigned long long)is.shifted,
                (unsigned long long)is.low_qual);
        check(h, real_hip_indel_end(h), "real_hip_indel_end");
    }
    check(h, real_hip_call_end(h), "real_hip_call_end");
}

// addAll(ctx, calls): every batch of reads with its final records to the pileup (calls = false) or to the calls on top of it
// gapAll(ctx, fi, leg): every batch of mates with its gap records to one leg -- kGapPileup (-pileup_gapped 1): through the gap
// rescue to real_hip_pileup_add_gapped, behind the ungapped adds and before the finish; kGapCalls: to real_hip_call_add_gapped
// (writeCalls); kGapIndels (-vcf_indels 1): to real_hip_indel_add, through the gap rescue unless kGapPileup has run it
template <class AddAll, class GapAll>
void pileupPass(const RealOptions &o, const std::vector<std::string> &files, const Ranges &RS, Timers &T, AddAll addAll, GapAll gapAll)
{
    if (!o.pileup_given && !o.pileup_depth_given && !o.vcf_given) return;
    std::unique_ptr<OutFile> sites_out(o.pileup_given ? new OutFile(o.pileupfilename, false, "-pileup") : nullptr);
    std::unique_ptr<OutFile> depth_out(o.pileup_depth_given ? new OutFile(o.pileupdepthfilename, false, "-pileup_depth") : nullptr);
    std::unique_ptr<OutFile> vcf_out(o.vcf_given ? new OutFile(o.vcffilename, false, "-vcf") : nullptr);
    const SamRefs refs(RS.names, RS.starts);
    if (vcf_out) {
        const std::string head = vcfHeader(refs, o.vcf_indels);
        if (fwrite(head.data(), 1, head.size(), vcf_out->file()) != head.size()) throw std::runtime_error("write to the -vcf file failed");
    }
    real_hip_pileup_params pp = sized<real_hip_pileup_params>();
    pp.min_qual = (uint32_t)o.pileup_minq;
    textPass(o, files, T, [&](CtxVec &ctx, unsigned fi, const GenomeText &G) {
        real_hip_ctx *h = ctx[0]->h;
        check(h, real_hip_pileup_begin(h, &pp), "real_hip_pileup_begin");
        addAll(ctx, false);
        if (o.pileup_gapped) gapAll(ctx, fi, kGapPileup);
        uint64_t n_sites = 0;
        check(h, real_hip_pileup_finish(h, &n_sites), "real_hip_pileup_finish");
        if (sites_out) writeSites(h, n_sites, G, sites_out->file());
        if (depth_out) writeDepthRuns(h, G, depth_out->file());
        const real_hip_pileup_stats st = readStats(h, real_hip_pileup_stats_get, 1, "real_hip_pileup_stats_get");
        fprintf(stderr, "pileup: file=%s placements=%llu bases=%llu covered=%llu mean_depth=%.3f max_depth=%llu sites=%llu mismatches=%llu low_qual=%llu\n",
                files[fi].c_str(), (unsigned long long)st.placed, (unsigned long long)st.bases, (unsigned long long)st.covered,
                st.covered ? (double)st.bases / (double)st.covered : 0.0, (unsigned long long)st.max_depth, (unsigned long long)st.sites,
                (unsigned long long)st.mismatches, (unsigned long long)st.low_qual);
        if (o.pileup_gapped) {
            const real_hip_pileup_gapped_stats gs = readStats(h, real_hip_pileup_gapped_stats_get, 1, "real_hip_pileup_gapped_stats_get");
            fprintf(stderr, "pileup gapped: file=%s placements=%llu ungapped=%llu aligned=%llu deleted=%llu inserted=%llu mismatches=%llu low_qual=%llu\n",
                    files[fi].c_str(), (unsigned long long)gs.placed, (unsigned long long)gs.ungapped, (unsigned long long)gs.aligned_bases,
                    (unsigned long long)gs.deleted, (unsigned long long)gs.inserted, (unsigned long long)gs.mismatches, (unsigned long long)gs.low_qual);
        }
        if (vcf_out) writeCalls(o, ctx, fi, files[fi], refs.names[fi], G, vcf_out->file(), addAll, gapAll);
        check(h, real_hip_pileup_end(h), "real_hip_pileup_end");
    });
    for (OutFile *f : {sites_out.get(), depth_out.get(), vcf_out.get()}) {
        if (!f) continue;
        const bool bad = ferror(f->file()) != 0; // (a line that could not be written)
        f->close();
        if (bad) throw std::runtime_error("write to the -pileup / -pileup_depth / -vcf file failed");
    }
}

// ---- -sam: every read as a SAM line, NM / MD from the mismatch lists of the final placements ----------------------------
// Runs where pileupPass runs, through the same textPass.  The header names the fragments of all genome files (RS).  Per file
// writeAll(ctx, fi, last, refs, lists, out) streams the reads once more, takes each batch's lists from real_hip_mismatches /
// _pairs with the final records (SamLists::add), and writes the lines of the reads placed in this file -- and, in the pass
// of the last file, of those placed nowhere (Sam.hpp: all about the lines).  A summary line per file goes to standard error.
// The lists of a batch and the protocol that fills them: list(h, in..., mm, room, &n, off) lists n_lists reads into mm.  A call
// that overflows has counted and written nothing: its statistics are dropped (read and reset through get) and the call is
// repeated with room for what it reported (and an eighth more).  Returns the statistics of the call that listed.
struct Lists {
    std::vector<real_hip_mismatch> mm = std::vector<real_hip_mismatch>(1024); // (grows by the count the library reports)
    std::vector<uint64_t> off;
    template <class Stats, class List, class... In>
    Stats fill(real_hip_ctx *h, const char *what, int (*get)(real_hip_ctx *, Stats *, int), const char *get_name, uint64_t n_lists, List list, In... in)
    {
        off.assign(n_lists + 1, 0);
        uint64_t n = 0;
        int rc = list(h, in..., mm.data(), mm.size(), &n, off.data());
        if (rc == REAL_HIP_E_OVERFLOW) {
            readStats(h, get, 1, get_name);
            mm.resize(n + n / 8 + 16);
            rc = list(h, in..., mm.data(), mm.size(), &n, off.data());
        }
        check(h, rc, what);
        return readStats(h, get, 1, get_name);
    }
};
// real_hip_mismatches / _pairs: the sums over a genome file
struct SamLists : Lists {
    uint64_t placed = 0, mismatches = 0, on_n = 0, disagree = 0;
    template <class List, class... In>
    void add(real_hip_ctx *h, const char *what, uint64_t n_lists, List list, In... in)
    {
        const real_hip_mismatch_stats st = fill(h, what, real_hip_mismatch_stats_get, "real_hip_mismatch_stats_get", n_lists, list, in...);
        placed += st.placed; mismatches += st.mismatches; on_n += st.on_n; disagree += st.disagree;
    }
};
// -sam_gapped 1: the lists of the mates the gap rescue placed, list i for fragment i of the batch (real_hip_mismatches_gapped);
// the stage's own statistics summed over the run
struct GappedLists : Lists {
    uint64_t mates = 0, deleted = 0, inserted = 0, disagree = 0;
    void add(real_hip_ctx *h, uint64_t n, const real_hip_batch *rb1, const real_hip_batch *rb2, const real_hip_gap_place *gaps)
    {
        const real_hip_gapped_list_stats st = fill(h, "real_hip_mismatches_gapped", real_hip_gapped_list_stats_get, "real_hip_gapped_list_stats_get", n,
                                                   real_hip_mismatches_gapped, rb1, rb2, gaps);
        mates += st.placed; deleted += st.deleted; inserted += st.inserted; disagree += st.disagree;
    }
};

template <class WriteAll>
void samPass(const RealOptions &o, const std::vector<std::string> &files, const Ranges &RS, Timers &T, WriteAll writeAll)
{
    if (!o.sam_given) return;
    const SamRefs refs(RS.names, RS.starts);
    OutFile out(o.samfilename, false, "-sam");
    const std::string head = refs.header();
    if (fwrite(head.data(), 1, head.size(), out.file()) != head.size()) throw std::runtime_error("write to the -sam file failed");
    SamLists L;
    textPass(o, files, T, [&](CtxVec &ctx, unsigned fi, const GenomeText &) {
        L.placed = L.mismatches = L.on_n = L.disagree = 0;
        writeAll(ctx, fi, fi + 1 == files.size(), refs, L, out.file());
        fprintf(stderr, "sam: file=%s placements=%llu mismatches=%llu on_n=%llu disagree=%llu\n", files[fi].c_str(), (unsigned long long)L.placed,
                (unsigned long long)L.mismatches, (unsigned long long)L.on_n, (unsigned long long)L.disagree);
    });
    out.close();
}

// ---- -dedup: the copies of a placed read / fragment marked (real_hip_mark_duplicates*) -------------------------
// The summaries are taken with the first pass over the reads and kept beside the records; behind "All done." one call marks
// all records on the first context (duplicates in different batches, host blocks and parser chunks meet), and the summary line
// goes to standard error.  The pileup then gets, per batch, a scratch copy of the records with the duplicates set to NoMatch.
// mark(): the driver's real_hip_mark_duplicates* call, which fills dup
template <class Mark>
void markDuplicates(real_hip_ctx *h, const RealOptions &o, Timers &T, uint64_t numpat, std::vector<uint8_t> &dup, Mark mark)
{
    dup.assign(numpat, 0);
    const double tm = now_s();
    mark();
    T.match += now_s() - tm;
    const real_hip_dup_stats st = readStats(h, real_hip_dup_stats_get, 1, "real_hip_dup_stats_get");
    fprintf(stderr, "duplicates: placed=%llu groups=%llu duplicates=%llu rate=%.4f min_qual=%ld\n", (unsigned long long)st.placed, (unsigned long long)st.groups,
            (unsigned long long)st.duplicates, st.placed ? (double)st.duplicates / (double)st.placed : 0.0, o.dedup_minq);
}
// records[first .. first + n) with the duplicates masked, in `scratch`; the records themselves where nothing is marked
template <class Rec, class Mask>
const Rec *withoutDuplicates(const std::vector<Rec> &records, const std::vector<uint8_t> &dup, uint64_t first, uint64_t n, std::vector<Rec> &scratch, Mask mask)
{
    if (dup.empty()) return records.data() + first;
    scratch.assign(records.begin() + (ptrdiff_t)first, records.begin() + (ptrdiff_t)(first + n));
    for (uint64_t i = 0; i < n; ++i)
        if (dup[first + i]) mask(scratch[i]);
    return scratch.data();
}

// ---- -mapq 1: the qualities of the final placements (real_hip_mapq*) ------------------------------------------
// The accumulators are kept for the run beside the records and fold over every index block and genome file; behind "All
// done.", where -dedup marks, one call on the first context turns them into one byte per read (two per fragment), and the
// summary line goes to standard error.  -sam writes the bytes; -pileup_minmapq masks with them as -dedup masks.
const real_hip_mapq_acc kNoCandidates = {INT32_MIN, 0, {0}};
// rate(): the driver's real_hip_mapq* call, which fills the n bytes of mapq
template <class Rate>
void rateMapq(real_hip_ctx *h, Timers &T, uint64_t n, std::vector<uint8_t> &mapq, Rate rate)
{
    mapq.assign(n, REAL_HIP_MAPQ_NONE);
    const double tm = now_s();
    rate();
    T.match += now_s() - tm;
    const real_hip_mapq_stats st = readStats(h, real_hip_mapq_stats_get, 1, "real_hip_mapq_stats_get");
    uint64_t sum = 0, placed = 0;
    for (const uint8_t q : mapq)
        if (q != REAL_HIP_MAPQ_NONE) { sum += q; ++placed; }
    fprintf(stderr, "mapq: placements=%llu unlisted=%llu mean=%.3f\n", (unsigned long long)st.placements, (unsigned long long)st.unlisted,
            placed ? (double)sum / (double)placed : 0.0);
}
// what the pileup leaves out: the duplicates, and with -pileup_minmapq the records i with below(i)
template <class Below>
std::vector<uint8_t> dropMask(const RealOptions &o, uint64_t numpat, const std::vector<uint8_t> &dup, Below below)
{
    std::vector<uint8_t> drop = dup;
    if (o.pileup_minmapq > 0) {
        drop.resize(numpat, 0);
        for (uint64_t i = 0; i < numpat; ++i)
            if (below(i)) drop[i] = 1;
    }
    return drop;
}

// ---- gap records: what -gapped (paired) and -gapped_single share -------------------------------------------------------------
real_hip_gap_params gapParams(const RealOptions &o)
{
    real_hip_gap_params gp = sized<real_hip_gap_params>();
    gp.max_gap = (uint32_t)o.gap_max; gp.min_flank = (uint32_t)o.gap_flank;
    gp.cost_mismatch = 4; gp.cost_open = 6; gp.cost_extend = 1; gp.max_cost = (uint32_t)o.gap_maxcost; gp.margin = (uint32_t)o.gap_margin;
    return gp;
}
// the record of a read without a gapped placement: NoMatch, as a call with fresh != 0 starts every record
inline real_hip_gap_place noGapRecord()
{
    real_hip_gap_place none;
    memset(&none, 0, sizeof none);
    none.second = REAL_HIP_GAP_NONE;
    return none;
}
// the CIGAR of a record of a read of patl bases ("*" where the library writes none)
struct Cigar { char s[48]; };
inline Cigar gapCigar(const real_hip_gap_place &g, uint64_t patl)
{
    Cigar c;
    strcpy(c.s, "*");
    real_hip_gap_cigar(&g, (uint32_t)patl, c.s, sizeof c.s);
    return c;
}
// The line of a Unique record in the -gapped / -gapped_single file: id, [mate 1|2,] strand, fragment, 1-based position, CIGAR,
// edit distance, mismatches, cost, the runner-up's cost or *[, the 1-based position of the anchor: the other mate].
inline void appendGapLine(std::string &s, const real_hip_gap_place &g, const ReadView &r, const Ranges &RS, int mate, const real_hip_single *anchor)
{
    char second[16] = "*", tail[160];
    if (g.second != REAL_HIP_GAP_NONE) snprintf(second, sizeof second, "%u", (unsigned)g.second);
    const int absg = g.gap < 0 ? -g.gap : g.gap;
    s.append(r.id, r.idlen);
    if (mate) s += mate == 2 ? "\t2" : "\t1";
    s += REAL_HIP_GAP_INVERTED(g.tag) ? "\t-\t" : "\t+\t";
    s += RS.names[g.fileid][g.frag];
    snprintf(tail, sizeof tail, "\t%llu\t%s\t%u\t%u\t%u\t%s", (unsigned long long)((uint64_t)g.pos - RS.starts[g.fileid][g.frag] + 1), gapCigar(g, r.patl).s,
             (unsigned)(g.k + absg), (unsigned)g.k, (unsigned)g.cost, second);
    s += tail;
    if (anchor) {
        snprintf(tail, sizeof tail, "\t%llu", (unsigned long long)((uint64_t)anchor->pos - RS.starts[anchor->fileid][anchor->frag] + 1));
        s += tail;
    }
    s += '\n';
}
// a batch's gap records to one leg of the pileup pass (pileupPass: gapAll)
void addGapLeg(real_hip_ctx *h, GapLeg leg, const real_hip_batch &rb1, const real_hip_batch &rb2, const real_hip_gap_place *gaps)
{
    if (leg == kGapPileup) check(h, real_hip_pileup_add_gapped(h, &rb1, &rb2, gaps), "real_hip_pileup_add_gapped");
    else if (leg == kGapCalls) check(h, real_hip_call_add_gapped(h, &rb1, &rb2, gaps), "real_hip_call_add_gapped");
    else check(h, real_hip_indel_add(h, &rb1, &rb2, gaps), "real_hip_indel_add");
}

// ---- -gapped_single: a single read placed nowhere, placed with one insertion or deletion (real_hip_match_gapped) ----
// Runs behind every other pass, on one fresh context on -device: every genome file and every index block of it once more
// (genomePass: the block loop of the matching passes, no one-block restriction), the reads through each block with their FINAL
// info words; the first block of the run starts the gap records, every other one folds into them.  Then the reads a last
// time for the ids: one line per Unique record, in read order, and the summary line on standard error.  eligible is the
// run's (the info words are final: it is the same in every block); anchored and crowded add up over the blocks -- a read
// counts once per block that anchors it; placed, unique and gapped count the final records.
// The pass has two halves.  The MATCHING half leaves the run's gap records; the WRITING half writes the file and the summary line.
// Without a consumer of the records both run here, on the pass's own context.  With one (-sam_gapped 1, -vcf_indels 1,
// -pileup_gapped 1 without -p2) the matching half runs behind "All done." on the matching contexts, before the
// marks of -dedup and the pileup and SAM passes, which read its records; the writing half stays here.
struct GapSingleRun {
    std::vector<real_hip_gap_place> gaps; // one record per read, from the matching half on
    uint64_t eligible = 0, anchored = 0, crowded = 0;
    bool matched = false;
};
// the matching half: every genome file and index block on the contexts gc (item g of a round on context g, as in the matching passes)
void gapSingleMatch(const RealOptions &o, CtxVec &gc, const std::vector<std::string> &files, Timers &T, int qoff, const std::vector<uint64_t> &info, uint64_t numpat,
                    GapSingleRun &run)
{
    const real_hip_gap_params gp = gapParams(o);
    real_hip_gap_anchor_params ap = sized<real_hip_gap_anchor_params>();
    ap.anchor_len = (uint32_t)o.gap_anchor; ap.max_anchors = (uint32_t)o.gap_anchors;
    run.gaps.assign(numpat, noGapRecord());
    bool first = true;
    for (unsigned fi = 0; fi < files.size(); ++fi) genomePass(o, gc, files, fi, 0, T, nullptr, [&](Resident &) {
        restreamReads(o, gc, qoff, false, T, numpat, &T.match, [&](size_t g, const ReadItem &it) {
            check(gc[g]->h, real_hip_match_gapped(gc[g]->h, &gp, &ap, &it.batch, info.data() + it.first_id, first ? 1 : 0, run.gaps.data() + it.first_id), "real_hip_match_gapped");
        });
        uint64_t eligible = 0;
        for (auto &c : gc) {
            const real_hip_gap_anchor_stats st = readStats(c->h, real_hip_gap_anchor_stats_get, 1, "real_hip_gap_anchor_stats_get");
            eligible += st.eligible;
            run.anchored += st.eligible - st.skipped - st.crowded - st.unanchored; run.crowded += st.crowded;
        }
        if (first) run.eligible = eligible;
        first = false;
    });
    run.matched = true;
}
void gapSinglePass(const RealOptions &o, const std::vector<std::string> &files, const Ranges &RS, Timers &T, int qoff, const std::vector<uint64_t> &info,
                   uint64_t numpat, GapSingleRun &run)
{
    if (!o.gapped_single_given) return;
    OutFile out(o.gappedsinglefilename, false, "-gapped_single");
    double t0 = now_s();
    CtxVec gc = makeContexts(o, 1);
    T.index += now_s() - t0;
    if (!run.matched) gapSingleMatch(o, gc, files, T, qoff, info, numpat, run);
    const std::vector<real_hip_gap_place> &gaps = run.gaps;
    uint64_t placed = 0, unique = 0, gapped = 0;
    restreamReads(o, gc, qoff, true, T, numpat, nullptr, [&](size_t, const ReadItem &it) {
        const ReadSource src = it.src;
        const uint64_t base = it.first_id;
        formatAndWrite(src.size(), out.file(), T, [&](uint64_t i, std::string &s) {
            const real_hip_gap_place &g = gaps[base + i];
            if (REAL_HIP_GAP_STATE(g.tag) == REAL_HIP_PAIR_UNIQUE) appendGapLine(s, g, src[i], RS, 0, nullptr);
        });
    });
    out.close();
    for (const real_hip_gap_place &g : gaps) {
        const unsigned st = REAL_HIP_GAP_STATE(g.tag);
        placed += st != REAL_HIP_PAIR_NOMATCH; unique += st == REAL_HIP_PAIR_UNIQUE; gapped += st != REAL_HIP_PAIR_NOMATCH && g.gap != 0;
    }
    std::cerr << "gap single: eligible=" << run.eligible << " anchored=" << run.anchored << " crowded=" << run.crowded << " placed=" << placed << " unique=" << unique
              << " gapped=" << gapped << std::endl;
}

// ---- EnumerateUniqueMatches::doMatching -------------------------------------------------
int matchUnique(const RealOptions &o)
{
    Timers T;
    const int qoff = qualityOffset(o, o.fastq, o.patternfilename);
    // uniqueinfo(numpat), :1094-1097.  The reference counts the reads in a pass of its own; here the arrays grow with the
    // first pass over the file (records start as NoMatch / -FLT_MAX, UniqueMatchInfo.hpp:191).
    std::vector<uint64_t> info;
    std::vector<float> score;
    std::vector<real_hip_read_sum> sums; // -dedup: kept for the run beside info
    std::vector<uint8_t> dup;            // -dedup: one mark per read, from behind "All done." on
    std::vector<real_hip_mapq_acc> acc;  // -mapq: kept for the run beside info
    std::vector<uint8_t> mapq;           // -mapq: one quality per read, from behind "All done." on
    uint64_t numpat = 0;
    bool counted = false;
    auto grow = [&](uint64_t n) {
        if (n > info.size()) {
            const uint64_t to = std::max<uint64_t>(n, info.size() + info.size() / 2);
            info.resize(to, 0);
            if (o.dedup) sums.resize(to);
            if (o.mapq) acc.resize(to, kNoCandidates);
            if (o.scores) score.resize(to, -FLT_MAX);
        }
    };
    const std::vector<std::string> files = genomeFiles(o, "more than 64 text files (6 bits of file id, UniqueMatchInfo.hpp:31)");
    CtxVec ctx = makeContexts(o);
    Ranges RS;
    for (unsigned fi = 0; fi < files.size(); ++fi) genomePass(o, ctx, files, fi, kSayLast, T, &RS, [&](Resident &) {
        const uint64_t seen = streamReads(o, ctx, qoff, false, T, [&](const std::vector<ReadItem> &items) {
            const uint64_t end = items.back().first_id + items.back().batch.n_reads;
            grow(end);
            const double tm = now_s();
            onEach(items.size(), [&](size_t g) {
                real_hip_batch rb = items[g].batch;
                rb.fresh = !counted; // first pass over the reads: the records start on the device
                if (rb.n_reads)
                    check(ctx[g]->h, real_hip_match_unique(ctx[g]->h, &rb, info.data() + items[g].first_id, o.scores ? score.data() + items[g].first_id : nullptr),
                          "real_hip_match_unique");
                if (o.dedup && !counted && rb.n_reads) // (the first pass over the reads: no pass of its own)
                    check(ctx[g]->h, real_hip_read_summary(ctx[g]->h, &rb, (uint32_t)o.dedup_minq, sums.data() + items[g].first_id), "real_hip_read_summary");
                if (o.mapq && rb.n_reads) // (every index block of every file: the candidates of a read are all its hits)
                    check(ctx[g]->h, real_hip_match_mapq(ctx[g]->h, &rb, acc.data() + items[g].first_id), "real_hip_match_mapq");
            });
            T.match += now_s() - tm;
            if (counted) std::cerr << "\r                                                              \r" << (double)end / (numpat ? numpat : 1) << std::flush;
        });
        if (!counted) { numpat = seen; counted = true; std::cerr << "number of reads " << numpat << std::endl; } // :1096
        else if (seen != numpat) throw std::runtime_error(kReadFileChanged);
        std::cerr << std::endl;
    });
    std::cerr << "All done." << std::endl;
    // the consumers of the gap records (single-end here: RealOptions has sorted out -p2, and each of them needs -gapped_single): with
    // one of them the matching half of the gapped pass runs now, on the matching contexts -- the only ones that hold an index
    const bool consumers = o.sam_gapped || o.vcf_indels || o.pileup_gapped;
    GapSingleRun gap_run;
    if (consumers) gapSingleMatch(o, ctx, files, T, qoff, info, numpat, gap_run);
    const std::vector<real_hip_gap_place> &gaps = gap_run.gaps;
    real_hip_ctx *h = ctx[0]->h;
    if (o.dedup) markDuplicates(h, o, T, numpat, dup, [&]() {
        if (consumers) // gapped and ungapped reads of one 5' end are one molecule's copies: one key space, one sort
            check(h, real_hip_mark_duplicates_gapped(h, info.data(), gaps.data(), sums.data(), numpat, 0, dup.data()), "real_hip_mark_duplicates_gapped");
        else
            check(h, real_hip_mark_duplicates(h, info.data(), sums.data(), numpat, 0, dup.data()), "real_hip_mark_duplicates");
    });
    if (o.dedup && consumers) {
        uint64_t placements = 0, marked = 0;
        for (uint64_t i = 0; i < numpat; ++i)
            if (REAL_HIP_GAP_STATE(gaps[i].tag) == REAL_HIP_PAIR_UNIQUE) { ++placements; marked += dup[i] != 0; }
        fprintf(stderr, "duplicates gapped: placements=%llu duplicates=%llu\n", (unsigned long long)placements, (unsigned long long)marked);
    }
    if (o.mapq) rateMapq(h, T, numpat, mapq, [&]() {
        check(h, real_hip_mapq(h, info.data(), o.scores ? score.data() : nullptr, acc.data(), numpat, 0, mapq.data()), "real_hip_mapq");
    });
    const std::vector<uint8_t> drop = dropMask(o, numpat, dup, [&](uint64_t i) { return mapq[i] != REAL_HIP_MAPQ_NONE && mapq[i] < o.pileup_minmapq; });
    // output, in read order (PatternIdReader re-stream, :1438-1486)
    OutFile out(o.outputfilename);
    uint64_t unique = 0;
    streamReads(o, ctx, qoff, true, T, [&](const std::vector<ReadItem> &items) {
        for (const ReadItem &it : items) { // (in file order)
            const ReadSource src = it.src;
            if (!src.size()) continue;
            const uint64_t base = it.first_id;
            formatAndWrite(src.size(), out.file(), T, [&](uint64_t i, std::string &s) {
                const Record r = unpack(info[base + i]);
                if (r.st != 1 && r.st != 2) return; // NoMatch / NonUnique / Gapped print nothing
                appendLine(s, src[i], o.scores, Placement{o.scores ? score[base + i] : 0.f, r.st == 2, RS.names[r.file][r.frag],
                                                          r.pos - RS.starts[r.file][r.frag] + 1, r.errors});
            });
        }
    });
    out.close();
    // (counted here, once, and not line by line inside the formatter: sixteen threads bumping neighbouring counters
    // cost more than formatting the lines)
#pragma omp parallel for reduction(+ : unique) schedule(static)
    for (uint64_t i = 0; i < numpat; ++i) { const unsigned st = (unsigned)(info[i] >> 61); unique += (st == 1 || st == 2); }
    std::cerr << "unique: " << unique << std::endl; // :1488
    if (passesBehindOutput(o)) ctx.clear(); // (the matching contexts go before the pass's own one comes)
    std::vector<uint64_t> kept; // -dedup / -pileup_minmapq: a batch's records without what they leave out
    std::vector<real_hip_gap_place> kept_gaps; // -dedup: a batch's gap records without the marked ones (-pileup_minmapq masks info words only)
    const real_hip_gap_place no_gap = noGapRecord();
    pileupPass(o, files, RS, T, [&](CtxVec &pc, bool calls) {
        restreamReads(o, pc, qoff, false, T, numpat, nullptr, [&](size_t, const ReadItem &it) {
            check(pc[0]->h, (calls ? real_hip_call_add : real_hip_pileup_add)(pc[0]->h, &it.batch, withoutDuplicates(info, drop, it.first_id, it.batch.n_reads, kept, [](uint64_t &r) { r = 0; })),
                  calls ? "real_hip_call_add" : "real_hip_pileup_add");
        });
    }, [&](CtxVec &pc, unsigned, GapLeg leg) { // (-pileup_gapped 1, -vcf_indels 1: the batch given as both mates, its gap records from the matching half)
        restreamReads(o, pc, qoff, false, T, numpat, nullptr, [&](size_t, const ReadItem &it) {
            const real_hip_gap_place *g = withoutDuplicates(gaps, dup, it.first_id, it.batch.n_reads, kept_gaps, [&](real_hip_gap_place &r) { r = no_gap; });
            const double tm = now_s();
            addGapLeg(pc[0]->h, leg, it.batch, it.batch, g);
            T.match += now_s() - tm;
        });
    });
    GappedLists GL; // -sam_gapped 1: the lists of the reads the gapped pass placed
    samPass(o, files, RS, T, [&](CtxVec &sc, unsigned fi, bool last, const SamRefs &refs, SamLists &L, FILE *sam) {
        restreamReads(o, sc, qoff, true, T, numpat, nullptr, [&](size_t, const ReadItem &it) {
            const uint64_t n = it.batch.n_reads, base = it.first_id;
            const double tm = now_s();
            L.add(sc[0]->h, "real_hip_mismatches", n, real_hip_mismatches, &it.batch, (const uint64_t *)info.data() + base);
            if (o.sam_gapped) GL.add(sc[0]->h, n, &it.batch, &it.batch, gaps.data() + base);
            T.match += now_s() - tm;
            const ReadSource src = it.src.withQuality(o.fastq, qoff);
            formatAndWrite(n, sam, T, [&](uint64_t i, std::string &s) {
                SamPlace at = samPlace(unpack(info[base + i]), o.scores ? score[base + i] : 0.f);
                at.duplicate = o.dedup && dup[base + i];
                if (o.mapq) at.mapq = mapq[base + i];
                if (o.sam_gapped && !at.placed && REAL_HIP_GAP_STATE(gaps[base + i].tag) == REAL_HIP_PAIR_UNIQUE) {
                    // placed by its gap record: a line as placed in the pass of the RECORD's file, and none as unplaced in the last one
                    const real_hip_gap_place &g = gaps[base + i];
                    if (g.fileid != fi) return;
                    const ReadView r = src[i];
                    const Cigar cigar = gapCigar(g, r.patl);
                    SamPlace p = samPlaceGapped(g, r.patl, cigar.s);
                    p.duplicate = at.duplicate;
                    appendSam(s, r, refs, p, nullptr, 0, 0, GL.mm.data() + GL.off[i], GL.off[i + 1] - GL.off[i], o.scores);
                    return;
                }
                appendSamRead(s, src[i], refs, at, fi, last, L.mm.data() + L.off[i], L.off[i + 1] - L.off[i], o.scores);
            });
        });
    });
    if (o.sam_gapped)
        fprintf(stderr, "sam gapped: reads=%llu deleted=%llu inserted=%llu disagree=%llu\n", (unsigned long long)GL.mates, (unsigned long long)GL.deleted,
                (unsigned long long)GL.inserted, (unsigned long long)GL.disagree);
    gapSinglePass(o, files, RS, T, qoff, info, numpat, gap_run);
    T.finish(numpat, unique);
    return EXIT_SUCCESS;
}

// ---- EnumerateAllMatches::doMatching ----------------------------------------------------
// Hits are emitted per genome block (matchAllImplementation.cpp:451-535).  The read blocks of a round go to the
// contexts in parallel; their lines are written in read order.
int matchAll(const RealOptions &o)
{
    Timers T;
    const int qoff = qualityOffset(o, o.fastq, o.patternfilename);
    const std::vector<std::string> files = genomeFiles(o, nullptr);
    CtxVec ctx = makeContexts(o);
    OutFile out(o.outputfilename);
    uint64_t n_reads = 0, n_lines = 0;
    for (unsigned fi = 0; fi < files.size(); ++fi) genomePass(o, ctx, files, fi, 0, T, nullptr, [&](Resident &R) {
        std::vector<std::vector<real_hip_hit>> hits(ctx.size(), std::vector<real_hip_hit>(1u << 20));
        std::vector<std::vector<uint64_t>> hoff(ctx.size());
        n_reads = streamReads(o, ctx, qoff, true, T, [&](const std::vector<ReadItem> &items) {
            const double tm = now_s();
            onEach(items.size(), [&](size_t g) {
                const real_hip_batch &rb = items[g].batch;
                hoff[g].assign(rb.n_reads + 1, 0);
                if (rb.n_reads) listGrowing(ctx[g]->h, "real_hip_match_all", hits[g], hoff[g].data(), real_hip_match_all, &rb);
            });
            T.match += now_s() - tm;
            for (size_t g = 0; g < items.size(); ++g) { // (in file order)
                const ReadSource src = items[g].src;
                const uint64_t n = src.size();
                if (!n) continue;
                n_lines += hoff[g][n];
                formatAndWrite(n, out.file(), T, [&](uint64_t i, std::string &s) {
                    const ReadView r = src[i];
                    for (uint64_t k = hoff[g][i]; k < hoff[g][i + 1]; ++k) {
                        const real_hip_hit &M = hits[g][k];
                        appendLine(s, r, o.scores, Placement{M.score, M.inverted != 0, R.G.frag_names[M.frag], (uint64_t)M.pos - R.G.frag_start[M.frag] + 1, M.k});
                    }
                });
            }
        });
    });
    out.close();
    std::cerr << "All done." << std::endl;
    T.finish(n_reads, n_lines);
    return EXIT_SUCCESS;
}

// ---- paired-end reads: what the two drivers share (no counterpart in the reference) --------------------------
real_hip_pair_params pairParams(const RealOptions &o)
{
    real_hip_pair_params pp = sized<real_hip_pair_params>();
    pp.min_insert = o.insert_min; pp.max_insert = o.insert_max; pp.orientation = 0;
    return pp;
}

// The two mate files of a run and the blocks their reads pass through (a ReadSource made of b1 / b2 follows them).
struct MateFiles {
    const RealOptions &o;
    int qoff1, qoff2;
    ReadBlock &b1, &b2;
};
const char *const kReadFilesChanged = "the read files changed between two passes";
// One pass over the two mate files from their start, the next block of each read in step by the host reader: read i of each
// are mates.  onBatch(first, n, rb1, rb2) runs with every batch -- fragments [first, first + n) of the run, in M.b1 / M.b2 and
// as the batches rb1 / rb2.  limit: at most so many fragments (the probe of -insert_auto), 0: all.  read_s, where given,
// receives the time spent in the reader.  again: a later pass, in which files that disagree have changed.  Returns the number
// of fragments seen.
template <class OnBatch>
uint64_t streamMates(const MateFiles &M, bool want_ids, uint64_t limit, double *read_s, bool again, OnBatch onBatch)
{
    const RealOptions &o = M.o;
    ReadReader r1(o.patternfilename, o.fastq, M.qoff1), r2(o.pattern2filename, o.fastq2, M.qoff2);
    uint64_t seen = 0;
    while (!limit || seen < limit) {
        const uint64_t room = limit ? std::min<uint64_t>(o.batch_reads, limit - seen) : o.batch_reads;
        const double t0 = now_s();
        const uint64_t n = r1.fillBlock(M.b1, room, want_ids), n2 = r2.fillBlock(M.b2, room, want_ids);
        if (read_s) *read_s += now_s() - t0;
        if (n != n2 && again) throw std::runtime_error(kReadFilesChanged);
        if (n != n2) throw std::runtime_error("the two read files hold different numbers of reads (" + o.patternfilename + ", " + o.pattern2filename + ")");
        if (!n) break;
        onBatch(seen, n, makeBatch(M.b1), makeBatch(M.b2));
        seen += n;
    }
    return seen;
}
// a later pass, which must find the numpat fragments the first pass counted
template <class OnBatch>
void restreamMates(const MateFiles &M, bool want_ids, uint64_t numpat, OnBatch onBatch)
{
    const uint64_t seen = streamMates(M, want_ids, 0, nullptr, true, [&](uint64_t first, uint64_t n, const real_hip_batch &rb1, const real_hip_batch &rb2) {
        if (first + n > numpat) throw std::runtime_error(kReadFilesChanged);
        onBatch(first, n, rb1, rb2);
    });
    if (seen != numpat) throw std::runtime_error(kReadFilesChanged);
}

// the lengths of a block's reads, from its offsets
void readLengths(const ReadBlock &b, std::vector<uint32_t> &len)
{
    len.resize(b.size());
    for (uint64_t i = 0; i < b.size(); ++i) len[i] = (uint32_t)(b.offsets[i + 1] - b.offsets[i]);
}

// The two lines of a pair (a real_hip_pair or a real_hip_pair_hit): mate 1, then mate 2 on the other strand; fs is the
// start of the fragment `fragname` in its file's text.
template <class Pair>
inline void appendPair(std::string &s, const ReadView &m1, const ReadView &m2, bool scores, const Pair &P, const std::string &fragname, uint64_t fs)
{
    appendLine(s, m1, scores, Placement{P.score1, P.inverted1 != 0, fragname, (uint64_t)P.pos1 - fs + 1, P.k1});
    appendLine(s, m2, scores, Placement{P.score2, P.inverted1 == 0, fragname, (uint64_t)P.pos2 - fs + 1, P.k2});
}

// ---- paired-end reads: one placement per fragment ---------------------------------------------------------
// Per genome file real_hip_match_pairs (-mate_search 1: real_hip_match_pairs_search) folds into the fragments' in/out
// records, as uniqueinfo[] folds for matchUnique.
// A Unique fragment prints the 11-column line of mate 1 and then of mate 2; NoMatch / NonUnique print nothing.
// ---- -gapped: the mate of a fragment without a pair, placed with one insertion or deletion (real_hip_gap_rescue) ----
// Runs where samPass runs, through the same textPass: per genome file the reads once more, each batch with its FINAL records;
// the first file starts the gap records, the others fold into them.  Then the reads a last time for the ids: one line per Unique
// record, in read order, and the summary line on standard error.
// -sam_gapped 1: the rescue of a genome file has run with that file's -sam pass (GapRun::rescue, every record started NoMatch,
// every file folded into them: the same array), so the records and the summed counters are already here and no pass is run.
// the gap records of the run and the counters of its rescue calls
struct GapRun {
    std::vector<real_hip_gap_place> gaps;
    real_hip_gap_stats sum;
    bool rescued = false; // the -sam pass ran the rescue
    GapRun() { memset(&sum, 0, sizeof sum); }
    void start(uint64_t numpat) { gaps.assign(numpat, noGapRecord()); }
    void addStats(real_hip_ctx *h)
    {
        const real_hip_gap_stats st = readStats(h, real_hip_gap_stats_get, 1, "real_hip_gap_stats_get");
        sum.eligible += st.eligible; sum.placed += st.placed; sum.unique += st.unique; sum.gapped += st.gapped;
    }
};
void gapPass(const RealOptions &o, const std::vector<std::string> &files, const Ranges &RS, Timers &T, const real_hip_pair_params &pp,
             const std::vector<real_hip_pair> &pairs, const std::vector<real_hip_single> &singles1, const std::vector<real_hip_single> &singles2,
             uint64_t numpat, const MateFiles &M, GapRun &run)
{
    if (!o.gapped_given) return;
    OutFile out(o.gappedfilename, false, "-gapped");
    const real_hip_gap_params gp = gapParams(o);
    if (!run.rescued) run.start(numpat); // (the first file's calls have fresh != 0: they ignore what the records hold and start each of them so)
    std::vector<real_hip_gap_place> &gaps = run.gaps;
    real_hip_gap_stats &sum = run.sum;
    if (!run.rescued) textPass(o, files, T, [&](CtxVec &gc, unsigned fi, const GenomeText &) {
        real_hip_ctx *h = gc[0]->h;
        restreamMates(M, false, numpat, [&](uint64_t seen, uint64_t, const real_hip_batch &rb1, const real_hip_batch &rb2) {
            const double tm = now_s();
            check(h, real_hip_gap_rescue(h, &pp, &gp, &rb1, &rb2, pairs.data() + seen, singles1.data() + seen, singles2.data() + seen, fi == 0, gaps.data() + seen),
                  "real_hip_gap_rescue");
            T.match += now_s() - tm;
        });
        run.addStats(h);
    });
    const ReadSource m1(M.b1), m2(M.b2);
    restreamMates(M, true, numpat, [&](uint64_t base, uint64_t n, const real_hip_batch &, const real_hip_batch &) {
        formatAndWrite(n, out.file(), T, [&](uint64_t i, std::string &s) {
            const real_hip_gap_place &g = gaps[base + i];
            if (REAL_HIP_GAP_STATE(g.tag) != REAL_HIP_PAIR_UNIQUE) return;
            const unsigned tm = REAL_HIP_GAP_TARGET(g.tag);
            appendGapLine(s, g, tm ? m2[i] : m1[i], RS, tm ? 2 : 1, tm ? &singles1[base + i] : &singles2[base + i]); // the anchor: the other mate
        });
    });
    out.close();
    std::cerr << "gap rescue: eligible=" << sum.eligible << " placed=" << sum.placed << " unique=" << sum.unique << " gapped=" << sum.gapped << std::endl;
}

// -unpaired <file>: real_hip_match_pairs_singles folds each mate's own hits beside the pairs; a fragment whose final pair
// state is NoMatch writes to <file> the line of mate 1 if it is Unique on its own, then mate 2's likewise, as the
// single-end mode would print that hit.  The main output does not change.
// -insert_hist <file>: the histogram of the final Unique records' outer distances (real_hip_pair_insert_hist in the output
// pass) as lines outer<TAB>count, its quartiles on standard error.  -insert_auto N: the bounds of the run come from the
// first N fragments against the first genome file (real_hip_insert_bounds), cut to -insert_min .. -insert_max.
int matchPairs(const RealOptions &o)
{
    Timers T;
    const int qoff1 = qualityOffset(o, o.fastq, o.patternfilename), qoff2 = qualityOffset(o, o.fastq2, o.pattern2filename);
    const std::vector<std::string> files = genomeFiles(o, "more than 64 text files");
    CtxVec ctx = makeContexts(o);
    real_hip_ctx *h = ctx[0]->h;
    real_hip_pair_params pp = pairParams(o); // (-insert_auto narrows the bounds before the first batch of the run)
    real_hip_mate_search_params sp = sized<real_hip_mate_search_params>(); // -mate_search 1: the search behind the join
    sp.max_anchors = o.mate_search_anchors;
    std::vector<real_hip_pair> pairs;
    const bool unpaired = !o.unpairedfilename.empty();
    const bool singles = unpaired || o.sam_given || o.mapq || o.gapped_given || o.vcf_indels || o.pileup_gapped; // (-sam places the mates of a fragment without a pair as -unpaired prints them; -mapq rates them; -gapped and -vcf_indels 1 take the rescue's anchors from them)
    std::vector<real_hip_single> singles1, singles2; // -unpaired / -sam: kept across the genome files as pairs is
    std::vector<real_hip_read_sum> sums1, sums2;     // -dedup: the mates' summaries, kept for the run beside pairs
    std::vector<uint8_t> dup;                        // -dedup: one mark per fragment, from behind "All done." on
    std::vector<real_hip_mapq_acc> accp, acc1, acc2; // -mapq: the fragments' and the mates' accumulators, kept for the run beside pairs
    std::vector<uint8_t> mapq;                       // -mapq: two qualities per fragment, from behind "All done." on
    uint64_t numpat = 0;
    Ranges RS;
    ReadBlock b1, b2;
    const MateFiles M{o, qoff1, qoff2, b1, b2};
    // the call of a batch, for the run and for the probe of -insert_auto
    // (A: the three accumulators of -mapq 1, null for the probe)
    auto matchBatch = [&](const real_hip_batch &rb1, const real_hip_batch &rb2, real_hip_pair *P, real_hip_single *S1, real_hip_single *S2,
                          real_hip_mapq_acc *const A[3] = nullptr) {
        if (A) check(h, real_hip_match_pairs_mapq(h, &rb1, &rb2, &pp, o.mate_search ? &sp : nullptr, P, S1, S2, A[0], A[1], A[2]), "real_hip_match_pairs_mapq");
        else if (singles) check(h, real_hip_match_pairs_singles(h, &rb1, &rb2, &pp, o.mate_search ? &sp : nullptr, P, S1, S2), "real_hip_match_pairs_singles");
        else if (o.mate_search) check(h, real_hip_match_pairs_search(h, &rb1, &rb2, &pp, &sp, P), "real_hip_match_pairs_search");
        else check(h, real_hip_match_pairs(h, &rb1, &rb2, &pp, P), "real_hip_match_pairs");
    };
    // the histogram of the records P of the fragments in b1 / b2 (added to hist unless fresh)
    std::vector<uint32_t> len1, len2;
    auto insertHist = [&](const real_hip_pair *P, uint64_t n, bool fresh, std::vector<uint64_t> &hist) {
        readLengths(b1, len1); readLengths(b2, len2);
        check(h, real_hip_pair_insert_hist(h, P, len1.data(), len2.data(), n, 0, fresh, (uint32_t)hist.size(), hist.data()), "real_hip_pair_insert_hist");
    };
    // -insert_auto N: the first N fragments against the first genome file under the window -insert_min .. -insert_max; the
    // quartiles of their Unique outer distances give the bounds of the run
    auto estimateBounds = [&]() {
        std::vector<real_hip_pair> probe;
        std::vector<real_hip_single> ps1, ps2;
        std::vector<uint64_t> hist((size_t)o.insert_max + 2, 0);
        const uint64_t seen = streamMates(M, false, o.insert_auto, nullptr, false, [&](uint64_t first, uint64_t n, real_hip_batch rb1, real_hip_batch rb2) {
            probe.resize(n);
            if (singles) { ps1.resize(n); ps2.resize(n); }
            rb1.fresh = rb2.fresh = 1;
            matchBatch(rb1, rb2, probe.data(), ps1.data(), ps2.data());
            insertHist(probe.data(), n, first == 0, hist);
        });
        real_hip_insert_estimate est = sized<real_hip_insert_estimate>();
        const int rc = real_hip_insert_bounds(hist.data(), (uint32_t)hist.size(), REAL_HIP_INSERT_MIN_COUNT, 3, &est);
        if (rc == REAL_HIP_E_STATE)
            throw std::runtime_error("-insert_auto: only " + std::to_string(est.n) + " of the first " + std::to_string(seen) + " fragments are placed uniquely (" +
                                     std::to_string(REAL_HIP_INSERT_MIN_COUNT) + " are needed): give the bounds explicitly with -insert_min / -insert_max.");
        if (rc == REAL_HIP_E_OVERFLOW)
            throw std::runtime_error("-insert_auto: the third quartile of the outer distances lies beyond -insert_max: give the bounds explicitly with -insert_min / -insert_max.");
        if (rc) throw std::runtime_error("real_hip_insert_bounds failed");
        pp.min_insert = std::max(o.insert_min, est.low);
        pp.max_insert = std::min(o.insert_max, est.high);
        std::cerr << "insert size estimate: fragments=" << seen << " unique=" << est.n << " q1=" << est.q1 << " median=" << est.median << " q3=" << est.q3
                  << " bounds=[" << pp.min_insert << ", " << pp.max_insert << "]" << std::endl;
    };
    for (unsigned fi = 0; fi < files.size(); ++fi) genomePass(o, ctx, files, fi, kSayLast | kOneBlock, T, &RS, [&](Resident &) {
        if (fi == 0 && o.insert_auto) {
            const double tm = now_s();
            estimateBounds();
            T.match += now_s() - tm;
        }
        const uint64_t seen = streamMates(M, false, 0, &T.read, false, [&](uint64_t first, uint64_t n, real_hip_batch rb1, real_hip_batch rb2) {
            if (first + n > pairs.size()) pairs.resize(std::max<uint64_t>(first + n, pairs.size() + pairs.size() / 2));
            if (singles && pairs.size() > singles1.size()) { singles1.resize(pairs.size()); singles2.resize(pairs.size()); }
            if (o.dedup && pairs.size() > sums1.size()) { sums1.resize(pairs.size()); sums2.resize(pairs.size()); }
            if (o.mapq && pairs.size() > accp.size())
                for (auto *a : {&accp, &acc1, &acc2}) a->resize(pairs.size(), kNoCandidates);
            rb1.fresh = rb2.fresh = (fi == 0); // first genome file: the records start on the device
            real_hip_mapq_acc *const A[3] = {o.mapq ? accp.data() + first : nullptr, o.mapq ? acc1.data() + first : nullptr, o.mapq ? acc2.data() + first : nullptr};
            const double tm = now_s();
            matchBatch(rb1, rb2, pairs.data() + first, singles ? singles1.data() + first : nullptr, singles ? singles2.data() + first : nullptr, o.mapq ? A : nullptr);
            if (o.dedup && fi == 0) { // (the first pass over the reads: no pass of its own)
                check(h, real_hip_read_summary(h, &rb1, (uint32_t)o.dedup_minq, sums1.data() + first), "real_hip_read_summary");
                check(h, real_hip_read_summary(h, &rb2, (uint32_t)o.dedup_minq, sums2.data() + first), "real_hip_read_summary");
            }
            T.match += now_s() - tm;
        });
        if (fi == 0) { numpat = seen; std::cerr << "number of fragments " << numpat << std::endl; }
        else if (seen != numpat) throw std::runtime_error(kReadFilesChanged);
    });
    std::cerr << "All done." << std::endl;
    if (o.dedup) markDuplicates(h, o, T, numpat, dup, [&]() {
        check(h, real_hip_mark_duplicates_pairs(h, pairs.data(), sums1.data(), sums2.data(), numpat, 0, dup.data()), "real_hip_mark_duplicates_pairs");
    });
    if (o.mapq) rateMapq(h, T, 2 * numpat, mapq, [&]() {
        check(h, real_hip_mapq_pairs(h, pairs.data(), singles1.data(), singles2.data(), accp.data(), acc1.data(), acc2.data(), numpat, 0, mapq.data()), "real_hip_mapq_pairs");
    });
    // (both mates of a Unique fragment carry the fragment's quality: "either below" is "both below")
    const std::vector<uint8_t> drop = dropMask(o, numpat, dup, [&](uint64_t i) { return pairs[i].state == REAL_HIP_PAIR_UNIQUE && mapq[2 * i] < o.pileup_minmapq; });
    OutFile out(o.outputfilename);
    std::unique_ptr<OutFile> uout(unpaired ? new OutFile(o.unpairedfilename, true) : nullptr);
    uint64_t unique = 0;
    // -insert_hist <file>: the outer distances of the final Unique records, batch by batch (the last bin: what lies beyond the bounds)
    const bool insert_hist = !o.inserthistfilename.empty();
    std::vector<uint64_t> hist(insert_hist ? (size_t)pp.max_insert + 2 : 0, 0);
    FILE *hist_file = insert_hist ? fopen(o.inserthistfilename.c_str(), "wb") : nullptr; // (opened before the pass: a path that cannot be written fails here)
    if (insert_hist && !hist_file) throw std::runtime_error("cannot open the -insert_hist file " + o.inserthistfilename);
    // the line of a mate that is placed uniquely on its own, as the single-end mode prints that hit
    auto singleLine = [&](std::string &s, const ReadView &r, const real_hip_single &S) {
        if (REAL_HIP_SINGLE_STATE(S.tag) != REAL_HIP_PAIR_UNIQUE) return;
        appendLine(s, r, o.scores, Placement{S.score, REAL_HIP_SINGLE_INVERTED(S.tag) != 0, RS.names[S.fileid][S.frag],
                                             (uint64_t)S.pos - RS.starts[S.fileid][S.frag] + 1, REAL_HIP_SINGLE_K(S.tag)});
    };
    const ReadSource m1(b1), m2(b2);
    restreamMates(M, true, numpat, [&](uint64_t base, uint64_t n, const real_hip_batch &, const real_hip_batch &) {
        if (insert_hist) insertHist(pairs.data() + base, n, base == 0, hist);
        if (unpaired)
            formatAndWrite(n, uout->file(), T, [&](uint64_t i, std::string &s) {
                if (pairs[base + i].state != REAL_HIP_PAIR_NOMATCH) return;
                singleLine(s, m1[i], singles1[base + i]);
                singleLine(s, m2[i], singles2[base + i]);
            });
        formatAndWrite(n, out.file(), T, [&](uint64_t i, std::string &s) {
            const real_hip_pair &P = pairs[base + i];
            if (P.state != REAL_HIP_PAIR_UNIQUE) return;
            appendPair(s, m1[i], m2[i], o.scores, P, RS.names[P.fileid][P.frag], RS.starts[P.fileid][P.frag]);
        });
    });
    out.close();
    for (uint64_t i = 0; i < numpat; ++i) unique += pairs[i].state == REAL_HIP_PAIR_UNIQUE;
    std::cerr << "unique fragments: " << unique << std::endl;
    if (unpaired) {
        uout->close();
        uint64_t mates = 0;
        for (uint64_t i = 0; i < numpat; ++i)
            if (pairs[i].state == REAL_HIP_PAIR_NOMATCH)
                mates += (REAL_HIP_SINGLE_STATE(singles1[i].tag) == REAL_HIP_PAIR_UNIQUE) + (REAL_HIP_SINGLE_STATE(singles2[i].tag) == REAL_HIP_PAIR_UNIQUE);
        std::cerr << "unpaired mates: " << mates << std::endl;
    }
    if (insert_hist) {
        bool ok = true;
        for (size_t d = 0; d < hist.size(); ++d)
            if (hist[d]) ok = fprintf(hist_file, "%zu\t%llu\n", d, (unsigned long long)hist[d]) > 0 && ok;
        if ((fclose(hist_file) != 0) || !ok) throw std::runtime_error("write to the -insert_hist file failed");
        real_hip_insert_estimate est = sized<real_hip_insert_estimate>();
        const int rc = real_hip_insert_bounds(hist.data(), (uint32_t)hist.size(), REAL_HIP_INSERT_MIN_COUNT, 3, &est);
        if (rc == REAL_HIP_E_STATE)
            std::cerr << "insert size: fewer than " << REAL_HIP_INSERT_MIN_COUNT << " unique fragments (n=" << est.n << "), no quartiles" << std::endl;
        else if (rc == REAL_HIP_OK || rc == REAL_HIP_E_OVERFLOW)
            std::cerr << "insert size: n=" << est.n << " q1=" << est.q1 << " median=" << est.median << " q3=" << est.q3 << std::endl;
        else throw std::runtime_error("real_hip_insert_bounds failed");
    }
    if (passesBehindOutput(o)) ctx.clear(); // (the matching context goes before the pass's own one comes)
    std::vector<real_hip_pair> kept; // -dedup / -pileup_minmapq: a batch's records without what they leave out
    // the gap rescue runs once per run: with -pileup_gapped 1 or -vcf_indels 1 in the pileup pass of each genome file (the text is
    // resident: what the rescue needs; with both, the pileup's leg runs it and the indel leg finds the records), else with
    // -sam_gapped 1 in the -sam pass, else in gapPass; the later passes find the records made
    GapRun gap_run;
    const real_hip_gap_params gp = gapParams(o);
    if (o.vcf_indels || o.pileup_gapped || o.sam_gapped) { gap_run.start(numpat); gap_run.rescued = true; }
    pileupPass(o, files, RS, T, [&](CtxVec &pc, bool calls) {
        restreamMates(M, false, numpat, [&](uint64_t seen, uint64_t n, const real_hip_batch &rb1, const real_hip_batch &rb2) {
            check(pc[0]->h, (calls ? real_hip_call_add_pairs : real_hip_pileup_add_pairs)(pc[0]->h, &rb1, &rb2, withoutDuplicates(pairs, drop, seen, n, kept, [](real_hip_pair &P) { P.state = REAL_HIP_PAIR_NOMATCH; })),
                  calls ? "real_hip_call_add_pairs" : "real_hip_pileup_add_pairs");
        });
    }, [&](CtxVec &pc, unsigned, GapLeg leg) {
        real_hip_ctx *h = pc[0]->h;
        const bool rescue = leg == kGapPileup || (leg == kGapIndels && !o.pileup_gapped);
        restreamMates(M, false, numpat, [&](uint64_t seen, uint64_t, const real_hip_batch &rb1, const real_hip_batch &rb2) {
            const double tm = now_s();
            if (rescue)
                check(h, real_hip_gap_rescue(h, &pp, &gp, &rb1, &rb2, pairs.data() + seen, singles1.data() + seen, singles2.data() + seen, 0, gap_run.gaps.data() + seen),
                      "real_hip_gap_rescue");
            addGapLeg(h, leg, rb1, rb2, gap_run.gaps.data() + seen);
            T.match += now_s() - tm;
        });
        if (rescue) gap_run.addStats(h);
    });
    // -sam_gapped 1: the pass of a genome file rescues the fragments whose anchor lies in it (unless -vcf_indels 1 has done so), lists
    // the rescued mates in gapped coordinates and writes their lines; gapPass then finds the records made
    GappedLists GL;
    const bool sam_rescues = o.sam_gapped && !o.vcf_indels && !o.pileup_gapped;
    samPass(o, files, RS, T, [&](CtxVec &sc, unsigned fi, bool last, const SamRefs &refs, SamLists &L, FILE *sam) {
        const ReadSource v1 = m1.withQuality(o.fastq, qoff1), v2 = m2.withQuality(o.fastq2, qoff2);
        restreamMates(M, true, numpat, [&](uint64_t seen, uint64_t n, const real_hip_batch &rb1, const real_hip_batch &rb2) {
            const double tm = now_s();
            L.add(sc[0]->h, "real_hip_mismatches_pairs", 2 * n, real_hip_mismatches_pairs, &rb1, &rb2, (const real_hip_pair *)pairs.data() + seen,
                  (const real_hip_single *)singles1.data() + seen, (const real_hip_single *)singles2.data() + seen);
            if (o.sam_gapped) {
                if (sam_rescues)
                    check(sc[0]->h, real_hip_gap_rescue(sc[0]->h, &pp, &gp, &rb1, &rb2, pairs.data() + seen, singles1.data() + seen, singles2.data() + seen, 0,
                                                        gap_run.gaps.data() + seen), "real_hip_gap_rescue");
                GL.add(sc[0]->h, n, &rb1, &rb2, gap_run.gaps.data() + seen);
            }
            T.match += now_s() - tm;
            formatAndWrite(n, sam, T, [&](uint64_t i, std::string &s) {
                const ReadView r[2] = {v1[i], v2[i]};
                SamPlace at[2] = {samPlace(pairs[seen + i], singles1[seen + i], 0), samPlace(pairs[seen + i], singles2[seen + i], 1)};
                at[0].duplicate = at[1].duplicate = o.dedup && dup[seen + i]; // (a duplicate fragment is Unique: both mates have lines)
                if (o.mapq) { at[0].mapq = mapq[2 * (seen + i)]; at[1].mapq = mapq[2 * (seen + i) + 1]; }
                if (o.sam_gapped && REAL_HIP_GAP_STATE(gap_run.gaps[seen + i].tag) == REAL_HIP_PAIR_UNIQUE && gap_run.gaps[seen + i].fileid <= fi) { // (a later file's record: -vcf_indels 1 ran the rescue of every file first)
                    const real_hip_gap_place &g = gap_run.gaps[seen + i];
                    appendSamRescued(s, r, refs, at, g, gapCigar(g, r[REAL_HIP_GAP_TARGET(g.tag)].patl).s, fi, pp.min_insert, pp.max_insert, L.mm.data(), L.off.data(), i,
                                     GL.mm.data() + GL.off[i], GL.off[i + 1] - GL.off[i], o.scores);
                } else appendSamFragment(s, r, refs, at, fi, last, L.mm.data(), L.off.data(), i, o.scores);
            });
        });
        if (sam_rescues) gap_run.addStats(sc[0]->h);
    });
    if (o.sam_gapped)
        fprintf(stderr, "sam gapped: mates=%llu deleted=%llu inserted=%llu disagree=%llu\n", (unsigned long long)GL.mates, (unsigned long long)GL.deleted,
                (unsigned long long)GL.inserted, (unsigned long long)GL.disagree);
    gapPass(o, files, RS, T, pp, pairs, singles1, singles2, numpat, M, gap_run);
    T.finish(2 * numpat, 2 * unique);
    return EXIT_SUCCESS;
}

// ---- paired-end reads: every concordant pair of a fragment (-pairs_all 1) -----------------------------------------
// Per genome file, as matchAll emits per block: real_hip_match_pairs_all gives every concordant pair of two seed hits of
// every fragment; for every fragment in read order and every pair in the ABI's order (row-major over the two mates' hit
// lists) the 11-column line of mate 1 and then of mate 2 is printed.  There is no fold across genome files.
int matchPairsAll(const RealOptions &o)
{
    Timers T;
    const int qoff1 = qualityOffset(o, o.fastq, o.patternfilename), qoff2 = qualityOffset(o, o.fastq2, o.pattern2filename);
    const std::vector<std::string> files = genomeFiles(o, "more than 64 text files");
    CtxVec ctx = makeContexts(o);
    real_hip_ctx *h = ctx[0]->h;
    const real_hip_pair_params pp = pairParams(o);
    OutFile out(o.outputfilename);
    std::vector<real_hip_pair_hit> hits;
    std::vector<uint64_t> poff;
    uint64_t numpat = 0, n_pairs = 0;
    ReadBlock b1, b2;
    const MateFiles M{o, qoff1, qoff2, b1, b2};
    const ReadSource m1(b1), m2(b2);
    for (unsigned fi = 0; fi < files.size(); ++fi) genomePass(o, ctx, files, fi, kSayLast | kOneBlock, T, nullptr, [&](Resident &R) {
        const uint64_t seen = streamMates(M, true, 0, &T.read, false, [&](uint64_t, uint64_t n, const real_hip_batch &rb1, const real_hip_batch &rb2) {
            poff.assign(n + 1, 0);
            if (hits.size() < n + n / 4 + 1024) hits.resize(n + n / 4 + 1024); // (about one pair per fragment is the rule: room for a quarter more)
            const double tm = now_s();
            n_pairs += listGrowing(h, "real_hip_match_pairs_all", hits, poff.data(), real_hip_match_pairs_all, &rb1, &rb2, &pp);
            T.match += now_s() - tm;
            formatAndWrite(n, out.file(), T, [&](uint64_t i, std::string &s) {
                const ReadView v1 = m1[i], v2 = m2[i];
                for (uint64_t k = poff[i]; k < poff[i + 1]; ++k) {
                    const real_hip_pair_hit &P = hits[k];
                    appendPair(s, v1, v2, o.scores, P, R.G.frag_names[P.frag], R.G.frag_start[P.frag]);
                }
            });
        });
        if (fi == 0) { numpat = seen; std::cerr << "number of fragments " << numpat << std::endl; }
        else if (seen != numpat) throw std::runtime_error(kReadFilesChanged);
    });
    out.close();
    std::cerr << "All done." << std::endl;
    std::cerr << "concordant pairs: " << n_pairs << std::endl;
    T.finish(2 * numpat, 2 * n_pairs);
    return EXIT_SUCCESS;
}

} // namespace

int main(int argc, char *argv[])
{
    std::cerr << "This is real (MI355X read-matching path), ABI " << real_hip_abi_version() << "." << std::endl;
    try {
        RealOptions opts(argc, argv);
        if (!opts.pattern2filename.empty()) return opts.pairs_all ? matchPairsAll(opts) : matchPairs(opts);
        return opts.match_unique ? matchUnique(opts) : matchAll(opts);
    } catch (const std::bad_alloc &) {
        std::cerr << "Insufficient memory." << std::endl;
        return EXIT_FAILURE;
    } catch (const std::exception &e) {
        std::cerr << e.what() << std::endl;
        return EXIT_FAILURE;
    }
}
