/* oracle/ref_shim: stand-in for the TBB names the reference's placement scorer and tree routines mention.
 * TEST INFRASTRUCTURE ONLY (oracle/ref_driver.cpp is single-threaded): the two concurrent containers are the std
 * ones, and the reader-writer lock around the best-placement state does nothing. */
#pragma once
#include <unordered_map>
#include <unordered_set>
namespace tbb {
template <class K, class V> using concurrent_unordered_map = std::unordered_map<K, V>;
template <class K> using concurrent_unordered_set = std::unordered_set<K>;
struct queuing_rw_mutex {
    struct scoped_lock {
        void acquire(queuing_rw_mutex &, bool = true) {}
        void release() {}
    };
};
}  // namespace tbb
