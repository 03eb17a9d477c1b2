// The RCX_* environment switches: each pins an alternate schedule for a test ("Switches"); none changes results beyond
// the stated tolerances.  They are read ONCE, at the first call that asks for one, into process-wide storage -- a launch pays no getenv()
// walks of the environment -- and again only when rcx_reload_options() is called (tests flip a switch and reload).
// Header-only: inline functions with one shared table per process.
#pragma once
#include <stdlib.h>
#include <mutex>
#include <string>

namespace rcx {
namespace opt {

enum Id { FORCE_GENERIC, CPL, CPL14, CPL14_RL, CPT, CPT_CB, CPT16, UPADD_CPL, UPADD_CPT, NESTED, TRAIN_FUSED, BWD_FUSED, WGRAD_CPL, COUNT };

namespace detail {
inline const char* name_of(int i)
{
    static const char* const k[COUNT] = {"RCX_FORCE_GENERIC", "RCX_CPL", "RCX_CPL14", "RCX_CPL14_RL", "RCX_CPT", "RCX_CPT_CB", "RCX_CPT16",
                                         "RCX_UPADD_CPL", "RCX_UPADD_CPT", "RCX_NESTED", "RCX_TRAIN_FUSED", "RCX_BWD_FUSED", "RCX_WGRAD_CPL"};
    return k[i];
}
struct Table {
    std::string val[COUNT];
    std::once_flag once;
    void read()
    {
        for (int i = 0; i < COUNT; ++i) {
            const char* v = getenv(name_of(i));
            val[i] = v ? v : "";
        }
    }
};
inline Table& table() { static Table t; return t; }
}  // namespace detail

// the variable's value as of the last (re)load, "" when it is not set; the pointer stays valid until the next reload
inline const char* str(Id id)
{
    detail::Table& t = detail::table();
    std::call_once(t.once, [&] { t.read(); });
    return t.val[id].c_str();
}
inline bool off(Id id) { return str(id)[0] == '0'; }                              // "RCX_X=0": switched off
inline bool on(Id id) { const char* v = str(id); return *v && *v != '0'; }         // set to anything but "" / "0..."
inline int int_or(Id id, int dflt) { const char* v = str(id); return *v ? atoi(v) : dflt; }
inline void reload()
{
    detail::Table& t = detail::table();
    std::call_once(t.once, [&] { t.read(); });
    t.read();
}

// RCX_FORCE_GENERIC=1: no hand-written schedule applies anywhere -- every RecConv2d, single step and backward runs on the generic kernels
inline bool hand_kernels_off() { return on(FORCE_GENERIC); }

}  // namespace opt
}  // namespace rcx
