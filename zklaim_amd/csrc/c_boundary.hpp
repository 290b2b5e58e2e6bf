// c_boundary.hpp — the one guard around every extern "C" entry: nothing propagates through the C boundary.  Host only, no HIP headers
// (tests/c/c_boundary_test.cpp includes it alone, with set_error stubbed).
#pragma once
#include <exception>
#include <string>

namespace zk {

void set_error(const std::string &msg);

// fn()'s value; a throw becomes zkg_last_error "<name>: <what()>" (or "<name>: unexpected exception") and the entry's own error value
template <class R, class F> R c_boundary(const char *name, R on_error, F &&fn) {
    try { return fn(); }
    catch (const std::exception &e) { set_error(std::string(name) + ": " + e.what()); }
    catch (...) { set_error(std::string(name) + ": unexpected exception"); }
    return on_error;
}

}  // namespace zk
