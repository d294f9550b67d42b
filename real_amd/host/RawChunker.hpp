// RawChunker.hpp -- the read file as text chunks of whole records (Lines.hpp: Chunk), read ahead by a thread.
// A chunk ends behind a newline whose index is a multiple of the lines per record (4 FASTQ, 2 FASTA) -- only text in
// one-line-per-field form parses on the device, and only for such text the cuts are record boundaries; what lies behind
// the cut is carried into the next chunk.  The next chunk is read by a prefetch thread while the caller works on the
// current ones.
// Host code only: nothing here calls into the library.  Where the buffers come from is the caller's business: `real`
// passes real_hip_host_alloc / real_hip_host_free (pinned memory: the chunks cross PCIe by DMA), host_selftest malloc / free.
#pragma once
#include <fcntl.h>
#include <unistd.h>

#include <cstring>
#include <future>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "Lines.hpp"

class RawChunker {
public:
    typedef void *(*Alloc)(size_t);
    typedef void (*Free)(void *);
    RawChunker(const std::string &fn, bool fastq, size_t chunk_bytes, size_t n_buffers, Alloc alloc, Free free_buffer) : free_buffer_(free_buffer), lpr_(fastq ? 4 : 2)
    {
        fd_ = open(fn.c_str(), O_RDONLY);
        if (fd_ < 0) throw std::runtime_error("Unable to open pattern file.");
        for (size_t i = 0; i < n_buffers; ++i) {
            Chunk c;
            c.text = (char *)alloc(chunk_bytes);
            if (!c.text) throw std::bad_alloc();
            c.cap = chunk_bytes;
            pool_.push_back(c);
            free_.push_back((int)i);
        }
        prefetch();
    }
    ~RawChunker()
    {
        if (next_.valid()) next_.wait();
        for (auto &c : pool_) free_buffer_(c.text);
        if (fd_ >= 0) close(fd_);
    }
    // the next chunk (the caller's until it hands it back with release); false at the end of the file
    bool next(Chunk &out, double &wait_s)
    {
        if (!next_.valid()) prefetch();
        if (!next_.valid()) return false;
        const double t0 = now_s();
        const int got = next_.get(); // (an exception of the reader thread surfaces here)
        wait_s += now_s() - t0;
        if (got < 0) { done_ = true; return false; }
        out = pool_[(size_t)got];
        prefetch();
        return true;
    }
    void release(const Chunk &c)
    {
        for (size_t i = 0; i < pool_.size(); ++i)
            if (pool_[i].text == c.text) free_.push_back((int)i);
        prefetch();
    }
private:
    // (only the thread that owns the chunker calls this, and only while no read is in flight: the reader thread is the
    // only one that touches the file state then)
    void prefetch()
    {
        if (done_ || next_.valid() || free_.empty()) return;
        const int id = free_.back();
        free_.pop_back();
        next_ = std::async(std::launch::async, [this, id]() { return fill(id) ? id : -1; });
    }
    // reads the next chunk with kReaders threads (pread of a slice each, then the newlines of the slice are counted
    // while it is hot), cuts it behind the last newline whose index is a multiple of the lines per record
    bool fill(int id)
    {
        Chunk &c = pool_[(size_t)id];
        const size_t have = carry_.size();
        if (have > c.cap) throw std::runtime_error("a read record longer than the text chunk");
        if (have) memcpy(c.text, carry_.data(), have);
        c.file_offset = offset_;
        carry_.clear();
        const size_t want = eof_ ? 0 : c.cap - have;
        constexpr int kReaders = 4;
        size_t got_s[kReaders] = {0, 0, 0, 0}, nl_s[kReaders] = {0, 0, 0, 0};
        bool err = false;
        auto slice = [&](int k) {
            const size_t lo = want * (size_t)k / kReaders, hi = want * (size_t)(k + 1) / kReaders;
            size_t done = 0;
            while (lo + done < hi) {
                const ssize_t r = pread(fd_, c.text + have + lo + done, hi - lo - done, (off_t)(fpos_ + lo + done));
                if (r < 0) { err = true; break; }
                if (r == 0) break; // end of file
                done += (size_t)r;
            }
            got_s[k] = done;
            size_t nl = 0;
            const char *b = c.text + have + lo, *e = b + done;
            if (k == 0) b = c.text; // (the carry belongs to the first slice)
            for (const char *q = b; (q = (const char *)memchr(q, '\n', (size_t)(e - q))); ++q) nl++;
            nl_s[k] = nl;
        };
        if (want) {
            std::thread th[kReaders - 1];
            for (int k = 1; k < kReaders; ++k) th[k - 1] = std::thread(slice, k);
            slice(0);
            for (auto &t : th) t.join();
        } else {
            slice(0); // (nothing to read: the newlines of the carry)
        }
        if (err) throw std::runtime_error("reading the pattern file failed");
        size_t got = 0, lines = 0;
        for (int k = 0; k < kReaders; ++k) { got += got_s[k]; lines += nl_s[k]; } // (a short slice = the end of the file: the slices behind it are empty)
        fpos_ += got;
        if (got < want || !want) eof_ = true;
        c.size = have + got;
        if (!c.size) return false;
        if (!eof_) {
            // behind newline number lines - lines % lpr: walk back over the lines % lpr newlines of the incomplete record
            size_t back = lines % lpr_, cut = c.size;
            const char *q = c.text + c.size;
            for (size_t k = 0; k <= back; ++k) {
                q = (const char *)memrchr(c.text, '\n', (size_t)(q - c.text));
                if (!q) { cut = 0; break; }
                cut = (size_t)(q - c.text) + 1;
            }
            if (lines < lpr_ || !cut) throw std::runtime_error("a read record longer than the text chunk");
            carry_.assign(c.text + cut, c.text + c.size);
            c.size = cut;
        }
        offset_ += c.size;
        return true;
    }
    Free free_buffer_;
    int fd_ = -1;
    uint64_t fpos_ = 0; // file position behind the bytes read so far
    size_t lpr_;
    bool eof_ = false, done_ = false;
    uint64_t offset_ = 0;
    std::vector<char> carry_;
    std::vector<Chunk> pool_;
    std::vector<int> free_;
    std::future<int> next_;
};
