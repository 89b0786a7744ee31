// Internal definitions shared by the host and device halves of libplfem_hip.so.
#pragma once
#include <cstdio>
#include <memory>
#include <new>
#include <string>
#include <system_error>

#include "../../include/plfem.h"
#include "symbolic.h"

struct plfem_symbolic {
  plfem::Symbolic S;
};

namespace {

// The error text of a creator, which has no handle yet to carry it: into the caller's buffer.  Returns rc.
int write_err(char* err, int32_t errlen, const std::string& msg, int rc) {
  if (err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", msg.c_str());
  return rc;
}

// Owner of a handle under construction (its deleter has internal linkage: no new exported symbol)
template <class T>
struct Delete {
  void operator()(T* p) const { delete p; }
};
template <class T>
using Owned = std::unique_ptr<T, Delete<T>>;

// No C++ exception crosses the C ABI: every extern "C" function that can allocate or start host threads is a
// function-try-block whose handler returns host_failure(handle): PLFEM_EHOST, with the exception's kind and what() as
// the error text of the handle (of the creator's buffer; nullptr, 0: a call with no handle reports the status alone).
// The functions left outside cannot throw: plfem_destroy, plfem_symbolic_destroy, plfem_locator_destroy,
// plfem_last_error, plfem_locator_last_error, plfem_symbolic_info and the sizers plfem_overlap_work_bytes,
// plfem_gram_work_bytes, plfem_profile_gram_work_bytes, plfem_quartic_work_bytes, plfem_project_work_bytes,
// plfem_project_sampled_work_bytes, plfem_indicator_work_bytes.  (plfem_symbolic_create returns through
// plfem_symbolic_create_ex.)
// Call it inside a catch handler only: the exception in flight stays alive until that handler exits.
int host_failure(char* err, int32_t errlen) noexcept {
  const char* kind = "host exception: ";
  const char* what = "unknown";
  try {
    throw;
  } catch (const std::bad_alloc& e) {
    kind = "out of host memory: ";
    what = e.what();
  } catch (const std::system_error& e) {
    kind = "host system error: ";
    what = e.what();
  } catch (const std::exception& e) {
    what = e.what();
  } catch (...) {
  }
  if (err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s%s", kind, what);   // (no allocation here)
  return PLFEM_EHOST;
}
template <class Owner>
int host_failure(Owner* owner) noexcept {
  char msg[256];
  host_failure(msg, sizeof(msg));
  try {
    if (owner) owner->err = msg;
  } catch (...) {   // (no memory for the text: the status still tells)
  }
  return PLFEM_EHOST;
}

}  // namespace
