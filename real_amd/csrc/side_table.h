// side_table.h -- a table of records kept BESIDE the objects they belong to, keyed by the object's address: create on first
// use, find without create, drop.  One lock, one map.  ctx_side.h keeps the state of the stages behind the matcher in one,
// beside the real_hip_ctx; why it is not inside the ctx is said there.
// The map is never destroyed: a record may own device memory, and none is freed from a static destructor, behind the HIP
// runtime's own end.  What is still in the table at the end of the process stays.
// No HIP in here: tests/test_side_state_cpu.py compiles it with the host compiler.
#pragma once
#include <mutex>
#include <unordered_map>

template <typename T>
class RhSideTable {
public:
    // the record of `key`, made (T's default constructor) on first use
    T &at(const void *key)
    {
        std::lock_guard<std::mutex> g(lock_);
        T *&s = map_[key];
        if (!s) s = new T();
        return *s;
    }
    // the record of `key`, or null: nothing is made
    T *find(const void *key)
    {
        std::lock_guard<std::mutex> g(lock_);
        auto it = map_.find(key);
        return it == map_.end() ? nullptr : it->second;
    }
    // the entry goes and its record with it (destroyed outside the lock); a later at() of the same key makes a fresh one
    void drop(const void *key)
    {
        T *s = nullptr;
        {
            std::lock_guard<std::mutex> g(lock_);
            auto it = map_.find(key);
            if (it == map_.end()) return;
            s = it->second;
            map_.erase(it);
        }
        delete s;
    }

private:
    using Map = std::unordered_map<const void *, T *>;
    std::mutex lock_;
    Map &map_ = *new Map(); // (never deleted)
};
