// The C-boundary guard (zklaim_amd/csrc/c_boundary.hpp) on its own, set_error stubbed: a normal return passes through; a std::exception
// and any other throw become the entry's error value and "<name>: <what>" / "<name>: unexpected exception".  For an int and a pointer return.
#include "../../zklaim_amd/csrc/c_boundary.hpp"
#include <cstdio>
#include <stdexcept>

static std::string g_last;
static int g_sets = 0;
namespace zk { void set_error(const std::string &msg) { g_last = msg; ++g_sets; } }

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (last error \"%s\")\n", __LINE__, #cond, g_last.c_str()); ++failures; } } while (0)

int main() {
    int object = 0, fallback = 0;

    // normal return: the value, and no error set
    CHECK(zk::c_boundary("name", 1, [&] { return 42; }) == 42 && g_sets == 0);
    CHECK(zk::c_boundary<int *>("name", nullptr, [&] { return &object; }) == &object && g_sets == 0);
    CHECK(zk::c_boundary<int *>("name", &fallback, [&]() -> int * { return nullptr; }) == nullptr && g_sets == 0);

    // std::exception: on_error and "name: what()"
    g_last.clear();
    CHECK(zk::c_boundary("name", 7, [&]() -> int { throw std::runtime_error("x"); }) == 7 && g_last == "name: x" && g_sets == 1);
    g_last.clear();
    CHECK(zk::c_boundary<int *>("name", nullptr, [&]() -> int * { throw std::runtime_error("x"); }) == nullptr && g_last == "name: x" && g_sets == 2);
    g_last.clear();
    CHECK(zk::c_boundary<int *>("other", &fallback, [&]() -> int * { throw std::runtime_error("x"); }) == &fallback && g_last == "other: x");

    // anything else: on_error and "name: unexpected exception"
    g_last.clear();
    CHECK(zk::c_boundary("name", 2, [&]() -> int { throw 7; }) == 2 && g_last == "name: unexpected exception");
    g_last.clear();
    CHECK(zk::c_boundary<int *>("name", nullptr, [&]() -> int * { throw 7; }) == nullptr && g_last == "name: unexpected exception");

    // the callable runs exactly once
    int runs = 0;
    (void)zk::c_boundary("name", 1, [&] { ++runs; return 0; });
    CHECK(runs == 1);

    if (failures) return 1;
    std::printf("c_boundary ok\n");
    return 0;
}
