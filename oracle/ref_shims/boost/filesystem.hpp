// oracle/ref_shims/boost/filesystem.hpp - the few names of boost::filesystem that findFilesWithExtension in the
// reference's utils/basic_algorithms.h spells.  The harness never lists a folder: everything here aborts when run.
// TEST INFRASTRUCTURE ONLY, for oracle/ref_harness.cpp.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <string>

namespace boost {
namespace filesystem {

[[noreturn]] inline void ref_shim_abort() {
  std::fprintf(stderr, "ref_shims/boost/filesystem is a stub\n");
  std::abort();
}

class path {
 public:
  path() {}
  path(const std::string &s) : s_(s) {}
  path(const char *s) : s_(s) {}
  path extension() const { ref_shim_abort(); }
  std::string string() const { return s_; }
  bool operator==(const std::string &o) const { return s_ == o; }
 private:
  std::string s_;
};

class directory_entry {
 public:
  const filesystem::path &path() const { return p_; }
 private:
  filesystem::path p_;
};

class directory_iterator {
 public:
  directory_iterator() {}
  explicit directory_iterator(const filesystem::path &) { ref_shim_abort(); }
  bool operator!=(const directory_iterator &) const { return false; }
  directory_iterator &operator++() { return *this; }
  const directory_entry *operator->() const { return &e_; }
 private:
  directory_entry e_;
};

inline bool exists(const path &) { ref_shim_abort(); }
inline bool is_directory(const path &) { ref_shim_abort(); }
inline bool is_regular_file(const path &) { ref_shim_abort(); }

}  // namespace filesystem
}  // namespace boost
