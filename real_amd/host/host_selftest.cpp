// host_selftest -- dumps what the host side computes, for the CPU tests (no GPU needed):
//   host_selftest genome <g.fa> <outdir>          -> sym.u8 frag.u64 names.txt text.u64 wild.u64
//   host_selftest reads <reads> <fastq:0|1> <qoff> <outdir> -> bases.u8 qual.u8 off.u64 ids.txt (+ count, offset detect)
//   host_selftest index <g.fa> <seedl> <first> <max> <threads> <outdir> -> l<k>_sign.bin l<k>_pos.u32 meta.txt
//   host_selftest options <args...>               -> prints the parsed RealOptions
//   host_selftest pair_options <args...>          -> prints the parsed paired-end flags
//   host_selftest pairs_all_options <args...>     -> prints the parsed -pairs_all flag
//   host_selftest unpaired_options <args...>      -> prints the parsed -unpaired file ("." if none)
//   host_selftest gapped_options <args...>        -> prints the parsed -gapped file ("." if none), -gap_max, -gap_flank, -gap_maxcost, -gap_margin
//   host_selftest gapped_single_options <args...> -> prints the parsed -gapped_single file ("." if none), -gap_anchor, -gap_anchors, -gap_max, -gap_flank, -gap_maxcost, -gap_margin
//   host_selftest sam_gapped_options <args...>    -> prints the parsed -sam_gapped flag (0|1), the -sam and the -gapped file ("." if none)
//   host_selftest insert_options <args...>        -> prints the parsed -insert_hist file ("." if none), -insert_auto, -insert_min, -insert_max
//   host_selftest rowaddr <seedl>                 -> checks the row addressing of the pair and canonical tables (csrc/row_addr.h), prints ok
//   host_selftest plan                            -> the table plan (csrc/index_plan.h, rh_plan_tables) over a grid of seed lengths, requests,
//       prefix widths, entry counts and device sizes: a line "l request prefix_bits n_entries device_bytes no_rows -> pb layout" each
//   host_selftest records                         -> checks the decoders of the final records and of the gap records (csrc/final_record.h)
//       against records written through the public structs, prints ok or the first disagreement
//   host_selftest gap_grid <n>                    -> the geometry rule of a gapped placement in a text of n bases (csrc/final_record.h, rh_gap_fit)
//       over a grid of lengths, gaps, splits and positions: a line "L g j p fits d del" each
//   host_selftest lines <reads.fq> <outdir>      -> block.tsv chunk.tsv: a line per read, formatted from the host reader's blocks and from the text
//   host_selftest chunks <reads> <fastq:0|1> <capacity> <buffers> <out> -> <out>: the text chunks RawChunker cuts the read file into with
//       <buffers> buffers of <capacity> bytes (malloc / free), per chunk file_offset and size as u64 and then the bytes
//   host_selftest sam <dir> <fastq:0|1> <qoff> <scores:0|1> <paired:0|1> -> <dir>/block.sam chunk.sam: the -sam file of the reads <dir>/r1 (and r2)
//       from the records in <dir> (names.txt: a line "file<TAB>start<TAB>name" per fragment and one "file<TAB>n<TAB>" behind a file's
//       last; info.u64 score.f32, or pairs.bin s1.bin s2.bin; per genome file mm<fi>.bin moff<fi>.u64), formatted by Sam.hpp from
//       the host reader's blocks and (single-end) from the text
//   host_selftest sam_gapped <dir> <fastq:0|1> <qoff> <insert_min> <insert_max> -> <dir>/block.sam: the -sam file of `real -sam_gapped 1` for the
//       mates <dir>/r1 and r2: the files of the paired `sam` command and gaps.bin (the gap records), cigars.txt (a line per fragment: the
//       record's CIGAR, * without one), per genome file gmm<fi>.bin goff<fi>.u64 (the gapped lists)
//   host_selftest vcf_indels <dir>               -> <dir>/out.vcf: the -vcf file of `real -vcf_indels 1` for one genome file, from sym.u8, frag.u64,
//       names.txt (a fragment name per line), calls.bin (real_hip_call records) and indels.bin (real_hip_indel records), through Vcf.hpp
//   host_selftest vcf_indel_options <args...>     -> prints the parsed -vcf_indels flag (0|1), -vcf_minalt, -vcf_minqual, -vcf_mindepth
//   host_selftest pileup_gapped_options <args...> -> prints the parsed -pileup_gapped flag (0|1), -gap_max, -gap_flank
//   host_selftest single_gapped_options <args...> -> prints the parsed -sam_gapped, -vcf_indels, -pileup_gapped and -dedup flags (0|1) and the
//                                                    -gapped_single file ("." if none): the single-end consumers of the gap records
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>

#include "FastFormat.hpp"
#include "GenomeText.hpp"
#include "HostIndex.hpp"
#include "Lines.hpp"
#include "RawChunker.hpp"
#include "ReadReader.hpp"
#include "RealOptions.hpp"
#include "Sam.hpp"
#include "Vcf.hpp"
#include "final_record.h"
#include "index_plan.h"
#include "row_addr.h"
#include <vector>

template <typename T>
static void dump(const std::string &fn, const T *p, size_t n)
{
    std::ofstream o(fn.c_str(), std::ios::binary);
    o.write(reinterpret_cast<const char *>(p), n * sizeof(T));
}

template <typename T>
static std::vector<T> slurp(const std::string &fn)
{
    std::ifstream f(fn.c_str(), std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<T> v(raw.size() / sizeof(T));
    if (!v.empty()) memcpy(v.data(), raw.data(), v.size() * sizeof(T));
    return v;
}

// the -sam file from records and lists on disk, through the functions `real` formats with
static int samSelftest(const std::string &d, bool fastq, int qoff, bool scores, bool paired, bool gapped = false, uint64_t insert_min = 0,
                       uint64_t insert_max = 0)
{
    std::vector<std::vector<std::string>> names;
    std::vector<std::vector<uint64_t>> starts;
    std::ifstream nf((d + "/names.txt").c_str());
    for (std::string line; std::getline(nf, line);) {
        const size_t a = line.find('\t'), b = line.find('\t', a + 1);
        const size_t f = (size_t)atoi(line.substr(0, a).c_str());
        if (names.size() <= f) { names.resize(f + 1); starts.resize(f + 1); }
        starts[f].push_back(strtoull(line.substr(a + 1, b - a - 1).c_str(), 0, 10));
        if (b + 1 < line.size()) names[f].push_back(line.substr(b + 1)); // (the line behind a file's last fragment has no name: its start is n)
    }
    const SamRefs refs(names, starts);
    const std::vector<uint64_t> info = slurp<uint64_t>(d + "/info.u64");
    const std::vector<float> score = slurp<float>(d + "/score.f32");
    const std::vector<real_hip_pair> pairs = slurp<real_hip_pair>(d + "/pairs.bin");
    const std::vector<real_hip_single> s1 = slurp<real_hip_single>(d + "/s1.bin"), s2 = slurp<real_hip_single>(d + "/s2.bin");
    std::vector<real_hip_gap_place> gaps;
    std::vector<std::string> cigars;
    if (gapped) {
        gaps = slurp<real_hip_gap_place>(d + "/gaps.bin");
        std::ifstream cf((d + "/cigars.txt").c_str());
        for (std::string line; std::getline(cf, line);) cigars.push_back(line);
        if (gaps.size() != pairs.size() || cigars.size() != pairs.size()) return 5;
    }
    // the reads, whole: as one block of the host reader and (single-end) as one chunk of text with its spans
    ReadBlock b1, b2;
    ReadReader r1(d + "/r1", fastq, qoff);
    const uint64_t n = r1.fillBlock(b1, ~0ull, true);
    if (paired) { ReadReader r2(d + "/r2", fastq, qoff); if (r2.fillBlock(b2, ~0ull, true) != n) return 3; }
    std::vector<char> text;
    Spans sp;
    if (!paired) {
        std::ifstream f((d + "/r1").c_str(), std::ios::binary);
        text.assign((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        sp.off.push_back(0);
        for (size_t p = 0; p < text.size();) { // one line per field
            const char *idl = (const char *)memchr(&text[p], '\n', text.size() - p);
            const size_t seq = (size_t)(idl - text.data()) + 1;
            const size_t seq_end = (size_t)((const char *)memchr(&text[seq], '\n', text.size() - seq) - text.data());
            sp.id_start.push_back((uint32_t)(p + 1)); sp.id_len.push_back((uint32_t)(seq - 1 - (p + 1)));
            sp.off.push_back(sp.off.back() + (seq_end - seq));
            p = seq_end + 1;
            if (fastq) for (int k = 0; k < 2; ++k) p = (size_t)((const char *)memchr(&text[p], '\n', text.size() - p) - text.data()) + 1;
        }
        if (sp.id_start.size() != n) return 4;
    }
    Chunk ch;
    ch.text = text.data(); ch.size = ch.cap = text.size();
    for (int form = 0; form < (paired ? 1 : 2); ++form) {
        std::string out = refs.header();
        const ReadSource v1 = (form ? ReadSource(ch, sp) : ReadSource(b1)).withQuality(fastq, qoff), v2 = ReadSource(b2).withQuality(fastq, qoff);
        for (unsigned fi = 0; fi < names.size(); ++fi) {
            const std::vector<real_hip_mismatch> mm = slurp<real_hip_mismatch>(d + "/mm" + std::to_string(fi) + ".bin");
            const std::vector<uint64_t> moff = slurp<uint64_t>(d + "/moff" + std::to_string(fi) + ".u64");
            std::vector<real_hip_mismatch> gmm;
            std::vector<uint64_t> goff;
            if (gapped) { gmm = slurp<real_hip_mismatch>(d + "/gmm" + std::to_string(fi) + ".bin"); goff = slurp<uint64_t>(d + "/goff" + std::to_string(fi) + ".u64"); }
            const bool last = fi + 1 == names.size();
            for (uint64_t i = 0; i < n; ++i) {
                if (!paired) {
                    appendSamRead(out, v1[i], refs, samPlace(unpack(info[i]), scores ? score[i] : 0.f), fi, last, mm.data() + moff[i], moff[i + 1] - moff[i], scores);
                } else {
                    const ReadView r[2] = {v1[i], v2[i]};
                    const SamPlace at[2] = {samPlace(pairs[i], s1[i], 0), samPlace(pairs[i], s2[i], 1)};
                    if (gapped && REAL_HIP_GAP_STATE(gaps[i].tag) == REAL_HIP_PAIR_UNIQUE)
                        appendSamRescued(out, r, refs, at, gaps[i], cigars[i].c_str(), fi, insert_min, insert_max, mm.data(), moff.data(), i, gmm.data() + goff[i],
                                         goff[i + 1] - goff[i], scores);
                    else appendSamFragment(out, r, refs, at, fi, last, mm.data(), moff.data(), i, scores);
                }
            }
        }
        std::ofstream o((d + (form ? "/chunk.sam" : "/block.sam")).c_str(), std::ios::binary);
        o.write(out.data(), (std::streamsize)out.size());
    }
    return 0;
}

int main(int argc, char **argv)
{
    try {
        if (argc < 2) return 2;
        std::string cmd = argv[1];
        if (cmd == "sam" && argc == 7) return samSelftest(argv[2], atoi(argv[3]) != 0, atoi(argv[4]), atoi(argv[5]) != 0, atoi(argv[6]) != 0);
        if (cmd == "sam_gapped" && argc == 7)
            return samSelftest(argv[2], atoi(argv[3]) != 0, atoi(argv[4]), false, true, true, strtoull(argv[5], 0, 10), strtoull(argv[6], 0, 10));
        if (cmd == "genome" && argc == 4) {
            GenomeText G; G.load(argv[2]);
            std::string d = argv[3];
            dump(d + "/sym.u8", G.sym.data(), G.sym.size());
            dump(d + "/frag.u64", G.frag_start.data(), G.frag_start.size());
            std::ofstream n((d + "/names.txt").c_str());
            for (auto &s : G.frag_names) n << s << "\n";
            std::ofstream nb((d + "/names.bin").c_str(), std::ios::binary); // (names may hold any byte but NUL)
            for (auto &s : G.frag_names) { nb.write(s.data(), (std::streamsize)s.size()); nb.put('\0'); }
            std::vector<uint64_t> t, w; G.pack(t, w);
            dump(d + "/text.u64", t.data(), t.size()); dump(d + "/wild.u64", w.data(), w.size());
            return 0;
        }
        if (cmd == "reads" && argc == 6) {
            bool fq = atoi(argv[3]); int qoff = atoi(argv[4]); std::string d = argv[5];
            uint64_t cnt = ReadReader::countPatterns(argv[2], fq);
            int det = fq ? ReadReader::getOffset(argv[2]) : 0;
            ReadReader rr(argv[2], fq, qoff ? qoff : det);
            ReadBlock all, b; all.clear();
            std::ofstream ids((d + "/ids.txt").c_str());
            std::ofstream idb((d + "/ids.bin").c_str(), std::ios::binary);
            while (rr.fillBlock(b, 7, true)) { // tiny blocks: exercises the block boundaries
                for (uint64_t i = 0; i < b.size(); ++i) {
                    all.bases.insert(all.bases.end(), b.bases.begin() + b.offsets[i], b.bases.begin() + b.offsets[i + 1]);
                    all.qual.insert(all.qual.end(), b.qual.begin() + b.offsets[i], b.qual.begin() + b.offsets[i + 1]);
                    all.offsets.push_back(all.bases.size());
                    ids << b.ids[i] << "\n";
                    idb.write(b.ids[i].data(), (std::streamsize)b.ids[i].size()); idb.put('\0');
                }
            }
            dump(d + "/bases.u8", all.bases.data(), all.bases.size()); dump(d + "/qual.u8", all.qual.data(), all.qual.size());
            dump(d + "/off.u64", all.offsets.data(), all.offsets.size());
            std::ofstream m((d + "/meta.txt").c_str());
            m << cnt << " " << det << "\n";
            return 0;
        }
        if (cmd == "index" && argc == 8) {
            GenomeText G; G.load(argv[2]);
            unsigned l = atoi(argv[3]); uint64_t first = strtoull(argv[4], 0, 10), mx = strtoull(argv[5], 0, 10);
            int th = atoi(argv[6]); std::string d = argv[7];
            std::vector<uint32_t> w; enumerateWindows(G.sym, l, w);
            HostIndexBlock B; buildHostIndexBlock(G.sym, w, l, first, mx, th, B);
            for (int k = 0; k < 6; ++k) {
                char nm[64];
                snprintf(nm, sizeof nm, "/l%d_sign.bin", k);
                if (B.sig_bytes == 4) dump(d + nm, B.sign32[k].data(), B.sign32[k].size()); else dump(d + nm, B.sign64[k].data(), B.sign64[k].size());
                snprintf(nm, sizeof nm, "/l%d_pos.u32", k);
                dump(d + nm, B.pos[k].data(), B.pos[k].size());
            }
            std::ofstream m((d + "/meta.txt").c_str());
            m << B.n << " " << (B.have_next ? 1 : 0) << " " << B.sig_bytes << " " << w.size() << "\n";
            return 0;
        }
        if (cmd == "fmtcheck" && argc == 3) { // fastformat::fmt_g6 against printf's %g on argv[2] floats
            const uint64_t n = strtoull(argv[2], 0, 10);
            uint64_t bad = 0, s = 0x9E3779B97F4A7C15ull;
            auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
            auto check = [&](float f) {
                char a[64], b[64];
                const int la = fastformat::fmt_g6(f, a), lb = snprintf(b, sizeof b, "%g", (double)f);
                if (la != lb || memcmp(a, b, (size_t)la)) { if (bad++ < 20) { a[la] = 0; std::cerr << "fmt_g6 " << a << " != " << b << std::endl; } }
            };
            for (uint64_t i = 0; i < n; ++i) {
                const uint64_t r = next();
                uint32_t u = (uint32_t)r;
                float f;
                memcpy(&f, &u, 4);                                       // any bit pattern (nan, inf, denormals: the fallback)
                check(f);
                check((float)((double)(int64_t)(r >> 40) / 1000.0 - 8000.0)); // score-like values with a few decimals
                check((float)(int32_t)(r >> 44));                         // integers
                const int k = (int)((r >> 32) % 21) - 5;                   // around the powers of ten, from both sides
                double pw = 1; for (int j = 0; j < (k < 0 ? -k : k); ++j) pw *= 10;
                const double c = k < 0 ? 1 / pw : pw;
                float g = (float)c;
                uint32_t gu; memcpy(&gu, &g, 4);
                gu += (uint32_t)(r % 7) - 3; memcpy(&g, &gu, 4);
                check(g); check(-g);
                check((float)(c * 9.999995)); check((float)(c * 0.9999995)); check((float)(c * 1.2345675)); check((float)(c * 999999.5 / 1e5));
            }
            std::cout << bad << std::endl;
            return bad ? 1 : 0;
        }
        if (cmd == "plan" && argc == 2) {
            // rh_plan_tables as the library compiles it, over a grid that reaches every branch (big = 2^27 entries or more)
            const uint32_t ls[] = {8, 12, 16, 20, 24, 28, 32, 36, 48, 64}, pbs[] = {0, 5, 12, 13, 20, 28, 30};
            const uint64_t ns[] = {0, 1, 1000, 32000, 1ull << 20, (1ull << 27) - 1, 1ull << 27, 3000000000ull, (1ull << 32) - 1};
            const uint64_t devs[] = {16ull << 30, 288ull << 30, 1ull << 62};
            for (uint32_t l : ls) for (uint32_t req = 0; req < 4; ++req) for (uint32_t pb : pbs) for (uint64_t n : ns) for (uint64_t dev : devs)
                for (int nr = 0; nr < 2; ++nr) {
                    const RhTables t = rh_plan_tables(l, req, pb, n, dev, nr != 0);
                    printf("%u %u %u %llu %llu %d -> %u %u\n", l, req, pb, (unsigned long long)n, (unsigned long long)dev, nr, t.pb, (unsigned)t.layout);
                }
            return 0;
        }
        if (cmd == "rowaddr" && argc == 3) {
            // rh_sig_rcform / rh_canon / rh_row_addr as the library compiles them: the rc-form against a base-by-base
            // reverse complement; (list, signature) -> (table, row, group) a bijection at every group width (all signatures
            // up to seedl 12); the four paired lookups and the two canonical ones in the row and group the design says (all seeds up to seedl 12, two
            // million drawn ones beyond: seedl 32 is the benchmark's geometry, its shifts by 0 and full masks included)
            const uint32_t l = (uint32_t)atoi(argv[2]), q = l / 4; // q bases per segment
            if (l < 4 || l > 32 || l % 4) return 2;
            const uint64_t nsig = 1ull << l, smask = nsig - 1;
            auto rc_naive = [](uint64_t v, uint32_t bases) { uint64_t o = 0; for (uint32_t i = 0; i < bases; ++i) o |= (3 - ((v >> (2 * i)) & 3)) << (2 * (bases - 1 - i)); return o; };
            uint64_t rs = 0x9E3779B97F4A7C15ull;
            auto next = [&]() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs; };
            const bool all = l <= 12;
            uint64_t bad = 0;
            for (uint64_t i = 0, n = l <= 16 ? nsig : 2000000; i < n; ++i) {
                const uint32_t sg = (uint32_t)((l <= 16 ? i : (i < 4 ? (i & 1 ? smask : 0) ^ (i & 2 ? 1 : 0) : next())) & smask);
                const uint32_t r = rh_sig_rcform(sg, l);
                if (r != (uint32_t)rc_naive(sg, l / 2) || rh_sig_rcform(r, l) != sg) bad++;
            }
            for (uint32_t gbits = 1; gbits <= 4 && gbits < l; ++gbits) {
                const uint32_t pb = l - gbits;
                if (all) {
                    const uint64_t off[4] = {0, 2 * nsig, 4 * nsig, 5 * nsig};
                    std::vector<uint8_t> seen(6 * nsig, 0);
                    for (uint32_t la = 0; la < 6; ++la)
                        for (uint64_t sg = 0; sg < nsig; ++sg) {
                            const RhRowAddr a = rh_row_addr(la, (uint32_t)sg, l, gbits);
                            if (a.table > 3 || a.table != (la > 3 ? 5 - la : la) || a.row >= rh_table_rows(la, pb) || a.group >= (1u << gbits)) { bad++; continue; }
                            uint8_t &s = seen[off[a.table] + (((uint64_t)a.row << gbits) | a.group)];
                            if (s) bad++;
                            s = 1;
                        }
                    for (uint8_t s : seen) if (!s) bad++;
                    // canonical tables: a signature and its rc-form in one row, their groups apart in the `which` bit alone; a
                    // signature that is its own rc-form has the one group; the sort key of the build is row, then group
                    for (uint32_t la = 2; la < 4; ++la)
                        for (uint64_t sg = 0; sg < nsig; ++sg) {
                            const uint32_t rf = rh_sig_rcform((uint32_t)sg, l), half = 1u << (gbits - 1);
                            const RhRowAddr a = rh_row_addr(la, (uint32_t)sg, l, gbits), b = rh_row_addr(la, rf, l, gbits);
                            const RhCanon c = rh_sig_canon((uint32_t)sg, l), cr = rh_sig_canon(rf, l);
                            if (a.table != la || b.table != la || a.row != b.row || (a.group ^ b.group) != (rf == sg ? 0u : half)) bad++;
                            if (c.index != cr.index || c.self != (rf == sg) || c.index >> (l - 1) || (rf != sg && c.which == cr.which)) bad++;
                            if (rh_place_key(la, (uint32_t)sg, l, gbits) != ((a.row << gbits) | a.group)) bad++;
                        }
                }
                const uint64_t nseed = all ? 1ull << (2 * l) : 2000000;
                const uint64_t gm = (1ull << (2 * q)) - 1;
                for (uint64_t i = 0; i < nseed; ++i) {
                    const uint64_t seed = all ? i : next();
                    uint32_t m[4], r[4];
                    for (int k = 0; k < 4; ++k) m[k] = (uint32_t)((seed >> (2 * q * (3 - k))) & gm);
                    for (int k = 0; k < 4; ++k) r[k] = (uint32_t)rc_naive(m[3 - k], q);
                    static const int A[6] = {0, 0, 0, 1, 1, 2}, C[6] = {1, 2, 3, 2, 3, 3}; // rh_list_segs
                    auto sig = [&](const uint32_t *s, int la) { return (uint32_t)((((uint64_t)s[A[la]] << (2 * q)) | s[C[la]]) & smask); };
                    for (int k = 0; k < 2; ++k)
                        for (int st = 0; st < 2; ++st) { // this strand's list k and the other strand's list 5 - k: one row
                            const uint32_t *own = st ? r : m, *oth = st ? m : r;
                            const RhRowAddr a = rh_row_addr(k, sig(own, k), l, gbits), b = rh_row_addr(5 - k, sig(oth, 5 - k), l, gbits);
                            const uint32_t half = 1u << (gbits - 1);
                            if (a.table != b.table || a.row != b.row || (a.group & half) || b.group != (a.group | half)) bad++;
                        }
                    for (int k = 2; k < 4; ++k) { // both strands' list k: one row of its canonical table, the groups apart in `which` alone
                        const uint32_t sf = sig(m, k), sr = sig(r, k), half = 1u << (gbits - 1), h2 = l / 2;
                        const RhRowAddr a = rh_row_addr(k, sf, l, gbits), b = rh_row_addr(k, sr, l, gbits);
                        if (sr != rh_sig_rcform(sf, l) || a.table != (uint32_t)k || b.table != (uint32_t)k || a.row != b.row || a.row >= rh_table_rows(k, pb) ||
                            (a.group ^ b.group) != (sf == sr ? 0u : half)) bad++;
                        // (the matcher has rc(low half) as the other strand's high half: no bit reversal)
                        const RhCanon c = rh_canon(sf >> h2, sr >> h2, h2), d = rh_sig_canon(sf, l);
                        if (c.index != d.index || c.which != d.which || c.self != d.self || c.self != (sf == sr)) bad++;
                        if (rh_place_key(k, sf, l, gbits) != ((a.row << gbits) | a.group)) bad++;
                    }
                }
            }
            std::cout << (bad ? "bad " : "ok ") << bad << std::endl;
            return bad ? 1 : 0;
        }
        if (cmd == "records" && argc == 2) {
            // csrc/final_record.h as the library compiles it, against records written through the public structs and macros of
            // real_hip.h (pairs, singles) and info words that Lines.hpp's unpack reads back as the fields they were made of
            auto fail = [](const char *what, uint64_t a, uint64_t b, uint64_t c) { std::cout << "bad " << what << " " << a << " " << b << " " << c << std::endl; return 1; };
            const uint32_t positions[3] = {0u, 1u, 0xffffffffu}, files[4] = {0, 1, 63, 255};
            for (uint32_t state = 0; state < 3; ++state)
                for (uint32_t inv1 = 0; inv1 < 2; ++inv1)
                    for (uint32_t file : files)
                        for (uint32_t p1 : positions)
                            for (uint32_t p2 : positions) {
                                real_hip_pair r;
                                memset(&r, 0, sizeof r);
                                r.best = -3.0; r.second = -5.0; r.score1 = 1.f; r.score2 = 1.f;
                                r.pos1 = p1; r.pos2 = p2; r.frag = 0xfffe; r.fileid = (uint8_t)file; r.k1 = 3; r.k2 = 12;
                                r.inverted1 = (uint8_t)inv1; r.state = (uint8_t)state; r.reserved = 0xff; // (reserved is 0 in real records: the decoders must not look)
                                uint32_t w[10];
                                memcpy(w, &r, sizeof r);
                                const uint64_t id = (uint64_t)state << 40 | (uint64_t)inv1 << 32 | file;
                                if (rh_pair_state(w[9]) != state || rh_pair_inverted1(w[9]) != (inv1 != 0) || rh_pair_fileid(w[8]) != file ||
                                    rh_pair_k1(w[8]) != r.k1 || rh_pair_k2(w[9]) != r.k2) return fail("pair fields", id, p1, p2);
                                for (uint32_t mate = 0; mate < 2; ++mate) {
                                    uint32_t st = 99;
                                    const RhPlace c = rh_place_pair(w[4], w[5], w[8], w[9], mate, &st);
                                    if (st != state || c.place != (state == REAL_HIP_PAIR_UNIQUE) || c.inv != ((inv1 != 0) != (mate != 0)) || c.file != file ||
                                        c.k != (mate ? r.k2 : r.k1) || c.pos != (mate ? p2 : p1)) return fail("pair mate", id, p1, p2);
                                }
                            }
            for (uint32_t state = 0; state < 4; ++state) // every value REAL_HIP_SINGLE_STATE can give
                for (uint32_t inv = 0; inv < 2; ++inv)
                    for (uint32_t k = 0; k < 16; k += 15)
                        for (uint32_t file : files)
                            for (uint32_t p : positions) {
                                real_hip_single s;
                                memset(&s, 0, sizeof s);
                                s.score = 1.f; s.second = -2.f; s.pos = p; s.frag = 0xfffe; s.fileid = (uint8_t)file;
                                s.tag = (uint8_t)(k | inv << 4 | state << 5);
                                if (REAL_HIP_SINGLE_K(s.tag) != k || REAL_HIP_SINGLE_INVERTED(s.tag) != inv || REAL_HIP_SINGLE_STATE(s.tag) != state) return fail("single tag", state, inv, k);
                                uint32_t w[4];
                                memcpy(w, &s, sizeof s);
                                const RhPlace c = rh_place_single(w[2], w[3]);
                                if (c.place != (state == REAL_HIP_PAIR_UNIQUE) || c.inv != (inv != 0) || c.file != file || c.k != k || c.pos != p)
                                    return fail("single", (uint64_t)state << 8 | inv << 4 | k, file, p);
                            }
            const uint64_t ipos[4] = {0, 0xffffffffull, 1ull << 32, (1ull << 35) - 1};
            for (uint64_t state = 0; state < 5; ++state)
                for (uint64_t file = 0; file < 64; file += 63)
                    for (uint64_t err = 0; err < 16; err += 15)
                        for (uint64_t p : ipos) {
                            const uint64_t rec = state << 61 | 0xfffeull << 45 | err << 41 | file << 35 | p;
                            const Record u = unpack(rec);
                            if (u.st != state || u.frag != 0xfffe || u.errors != err || u.file != file || u.pos != p) return fail("info word", state, file, p);
                            const RhPlace c = rh_place_info(rec);
                            if (c.place != (u.st == 1 || u.st == 2) || c.inv != (u.st == 2) || c.file != u.file || c.k != u.errors || c.pos != u.pos)
                                return fail("info", state, file, p);
                        }
            // gap records: every state, both targets, both strands, the file ids, positions, splits, gaps and mismatch counts at
            // the ends of their ranges; cost and second are not the decoder's business
            const uint32_t splits[4] = {0u, 1u, 319u, 0xffffu};
            const int gapv[7] = {-128, -17, -1, 0, 1, 17, 127};
            for (uint32_t state = 0; state < 4; ++state)
                for (uint32_t target = 0; target < 2; ++target)
                    for (uint32_t inv = 0; inv < 2; ++inv)
                        for (uint32_t file : files)
                            for (uint32_t p1 : positions)
                                for (uint32_t j : splits)
                                    for (int g : gapv) {
                                        real_hip_gap_place r;
                                        memset(&r, 0, sizeof r);
                                        r.pos = p1; r.frag = (uint16_t)(0xfffe - state); r.fileid = (uint8_t)file;
                                        r.tag = (uint8_t)(target | 0x0eu | inv << 4 | state << 5 | 0x80u); // (the bits no macro reads are set: the decoder must not look)
                                        r.split = (uint16_t)j; r.gap = (int8_t)g; r.k = (uint8_t)(255 - file); r.cost = 0xfffd; r.second = 0xfffc;
                                        if (REAL_HIP_GAP_TARGET(r.tag) != target || REAL_HIP_GAP_INVERTED(r.tag) != inv || REAL_HIP_GAP_STATE(r.tag) != state)
                                            return fail("gap tag", state, target, inv);
                                        uint32_t w[4];
                                        memcpy(w, &r, sizeof r);
                                        const RhGapRecord c = rh_place_gap(w[0], w[1], w[2], w[3]);
                                        if (c.state != state || c.file != file || c.target != target || c.inv != inv || c.frag != r.frag || c.p != p1 || c.j != j ||
                                            c.g != g || c.k != r.k) return fail("gap record", (uint64_t)state << 8 | target << 4 | inv, p1, (uint64_t)(int64_t)g);
                                    }
            std::cout << "ok" << std::endl;
            return 0;
        }
        if (cmd == "gap_grid" && argc == 3) {
            // the geometry rule of a gapped placement (csrc/final_record.h, rh_gap_fit) over a grid, a line "L g j p fits d del" each:
            // the lengths at the ends of the range and round a word of 32 bases, every gap one beyond REAL_HIP_GAP_MAX on either
            // side, every split one beyond the read, spans that end one before, on and one behind the text's end, a far position
            const uint64_t n = strtoull(argv[2], 0, 10);
            const uint32_t lengths[7] = {1, 2, 31, 32, 33, 320, 321};
            std::string out;
            char line[96];
            for (uint32_t L : lengths)
                for (int g = -17; g <= 17; ++g)
                    for (uint32_t j = 0; j <= L + 1; ++j)
                        for (int e = -1; e <= 2; ++e) {
                            const uint32_t p = e == 2 ? 0xFFFFFF00u : (uint32_t)((int64_t)n + e - (int64_t)L - g);
                            const RhGapFit f = rh_gap_fit(L, g, j, p, n);
                            snprintf(line, sizeof line, "%u %d %u %u %u %u %u\n", L, g, j, p, f.fits, f.d, f.del);
                            out += line;
                        }
            fwrite(out.data(), 1, out.size(), stdout);
            return 0;
        }
        if (cmd == "lines" && argc == 4) {
            // Every read of a one-line-per-field FASTQ file formatted twice (Lines.hpp): from the host reader's blocks, and
            // from the file as one text chunk whose spans a newline scan finds here.  The placement of read r is a fixed
            // function of r (tests/test_host_cpp.py states it again): both strands, scores on and off, positions up to
            // 2^35 - 1, errors 0..15, a fragment name with a leading space.
            const std::string d = argv[3];
            const std::string names[3] = {" chr one", "two", " 3"};
            auto line = [&](const ReadSource &src, uint64_t first, uint64_t i, std::string &s) {
                const uint64_t r = first + i;
                uint64_t pos1 = (r * 0x9E3779B97F4A7C15ull) >> 29;
                if (r == 0) pos1 = (1ull << 35) - 1;
                if (r == 1) pos1 = 1;
                appendLine(s, src[i], r % 3 != 2, Placement{(float)((int64_t)(r * 7919 % 100003) - 50000) / 16.0f, (r & 1) != 0, names[r % 3], pos1, (unsigned)(r % 16)});
            };
            Timers T;
            FILE *fb = fopen((d + "/block.tsv").c_str(), "wb"), *fc = fopen((d + "/chunk.tsv").c_str(), "wb");
            if (!fb || !fc) return 1;
            ReadReader rr(argv[2], true, ReadReader::getOffset(argv[2]));
            ReadBlock b;
            const ReadSource blocks(b);
            while (rr.fillBlock(b, 7, true)) // tiny blocks: most of the thread ranges are empty
                formatAndWrite(blocks.size(), fb, T, [&](uint64_t i, std::string &s) { line(blocks, b.first_id, i, s); });
            std::ifstream in(argv[2], std::ios::binary);
            std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
            Chunk c;
            c.text = &text[0]; c.cap = c.size = text.size();
            Spans sp;
            sp.off.push_back(0);
            for (size_t at = 0, ln = 0; at < text.size(); ++ln) { // line 4k: '@' id, line 4k + 1: the sequence; a '\r' belongs to neither
                size_t nl = text.find('\n', at);
                if (nl == std::string::npos) nl = text.size();
                const size_t len = nl - at - (nl > at && text[nl - 1] == '\r' ? 1 : 0);
                if (ln % 4 == 0) { sp.id_start.push_back((uint32_t)at + 1); sp.id_len.push_back((uint32_t)len - 1); }
                if (ln % 4 == 1) sp.off.push_back(sp.off.back() + len);
                at = nl + 1;
            }
            const ReadSource chunk(c, sp);
            formatAndWrite(chunk.size(), fc, T, [&](uint64_t i, std::string &s) { line(chunk, 0, i, s); });
            return (fclose(fb) == 0) & (fclose(fc) == 0) ? 0 : 1;
        }
        if (cmd == "chunks" && argc == 7) {
            RawChunker rc(argv[2], atoi(argv[3]) != 0, strtoull(argv[4], 0, 10), strtoull(argv[5], 0, 10), malloc, free);
            std::ofstream out(argv[6], std::ios::binary);
            Chunk c;
            double wait_s = 0;
            while (rc.next(c, wait_s)) {
                const uint64_t head[2] = {c.file_offset, c.size};
                out.write((const char *)head, sizeof head);
                out.write(c.text, (std::streamsize)c.size);
                rc.release(c);
            }
            return out.good() ? 0 : 1;
        }
        if (cmd == "options") {
            RealOptions o(argc - 1, argv + 1);
            std::cout << o.textfilename << " " << o.patternfilename << " " << o.outputfilename << " " << o.seedkmax << " " << o.totalkmax << " "
                      << o.seedl << " " << o.match_unique << " " << o.scores << " " << o.qualityOffset << " " << o.filter_level << " "
                      << o.filter_mult << " " << o.fastq << " " << o.gpus << " " << o.host_index << "\n";
            return 0;
        }
        if (cmd == "pair_options") { // the paired-end flags: -p2 file ("." if none), its format, -insert_min, -insert_max, format of -p
            RealOptions o(argc - 1, argv + 1);
            std::cout << (o.pattern2filename.empty() ? "." : o.pattern2filename) << " " << o.fastq2 << " " << o.insert_min << " " << o.insert_max << " "
                      << o.fastq << "\n";
            return 0;
        }
        if (cmd == "mate_search_options") { // -mate_search, -mate_search_anchors
            RealOptions o(argc - 1, argv + 1);
            std::cout << o.mate_search << " " << o.mate_search_anchors << "\n";
            return 0;
        }
        if (cmd == "unpaired_options") { // -unpaired
            RealOptions o(argc - 1, argv + 1);
            std::cout << (o.unpairedfilename.empty() ? "." : o.unpairedfilename) << "\n";
            return 0;
        }
        if (cmd == "gapped_options") { // -gapped and its -gap_* flags
            RealOptions o(argc - 1, argv + 1);
            std::cout << (o.gappedfilename.empty() ? "." : o.gappedfilename) << " " << o.gap_max << " " << o.gap_flank << " " << o.gap_maxcost << " "
                      << o.gap_margin << "\n";
            return 0;
        }
        if (cmd == "gapped_single_options") { // -gapped_single and its -gap_* flags
            RealOptions o(argc - 1, argv + 1);
            std::cout << (o.gappedsinglefilename.empty() ? "." : o.gappedsinglefilename) << " " << o.gap_anchor << " " << o.gap_anchors << " " << o.gap_max << " "
                      << o.gap_flank << " " << o.gap_maxcost << " " << o.gap_margin << "\n";
            return 0;
        }
        if (cmd == "sam_gapped_options") { // -sam_gapped
            RealOptions o(argc - 1, argv + 1);
            std::cout << (o.sam_gapped ? 1 : 0) << " " << (o.samfilename.empty() ? "." : o.samfilename) << " " << (o.gappedfilename.empty() ? "." : o.gappedfilename) << "\n";
            return 0;
        }
        if (cmd == "insert_options") { // -insert_hist, -insert_auto
            RealOptions o(argc - 1, argv + 1);
            std::cout << (o.inserthistfilename.empty() ? "." : o.inserthistfilename) << " " << o.insert_auto << " " << o.insert_min << " " << o.insert_max << "\n";
            return 0;
        }
        if (cmd == "pileup_gapped_options") { // -pileup_gapped
            RealOptions o(argc - 1, argv + 1);
            std::cout << (o.pileup_gapped ? 1 : 0) << " " << o.gap_max << " " << o.gap_flank << "\n";
            return 0;
        }
        if (cmd == "single_gapped_options") { // -sam_gapped / -vcf_indels / -pileup_gapped without -p2
            RealOptions o(argc - 1, argv + 1);
            std::cout << (o.sam_gapped ? 1 : 0) << " " << (o.vcf_indels ? 1 : 0) << " " << (o.pileup_gapped ? 1 : 0) << " " << (o.dedup ? 1 : 0) << " "
                      << (o.gappedsinglefilename.empty() ? "." : o.gappedsinglefilename) << "\n";
            return 0;
        }
        if (cmd == "vcf_indel_options") { // -vcf_indels, -vcf_minalt
            RealOptions o(argc - 1, argv + 1);
            std::cout << (o.vcf_indels ? 1 : 0) << " " << o.vcf_minalt << " " << o.vcf_minqual << " " << o.vcf_mindepth << "\n";
            return 0;
        }
        if (cmd == "vcf_indels" && argc == 3) { // the header and the merged lines of one genome file
            const std::string d = argv[2];
            const std::vector<uint8_t> sym = slurp<uint8_t>(d + "/sym.u8");
            const std::vector<uint64_t> frag = slurp<uint64_t>(d + "/frag.u64");
            const std::vector<real_hip_call> calls = slurp<real_hip_call>(d + "/calls.bin");
            const std::vector<real_hip_indel> indels = slurp<real_hip_indel>(d + "/indels.bin");
            std::vector<std::string> names;
            std::ifstream nf((d + "/names.txt").c_str());
            for (std::string line; std::getline(nf, line);) names.push_back(line);
            if (names.size() + 1 != frag.size()) throw std::runtime_error("names.txt and frag.u64 disagree");
            const SamRefs refs(std::vector<std::vector<std::string>>(1, names), std::vector<std::vector<uint64_t>>(1, frag));
            FILE *f = fopen((d + "/out.vcf").c_str(), "w");
            if (!f) throw std::runtime_error("cannot write out.vcf");
            const std::string head = vcfHeader(refs, true);
            fwrite(head.data(), 1, head.size(), f);
            writeVcfMerged(f, refs.names[0], frag.data(), sym.data(), calls.data(), calls.size(), indels.data(), indels.size());
            fclose(f);
            return 0;
        }
        if (cmd == "pairs_all_options") { // -pairs_all
            RealOptions o(argc - 1, argv + 1);
            std::cout << o.pairs_all << "\n";
            return 0;
        }
        return 2;
    } catch (const std::exception &e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
