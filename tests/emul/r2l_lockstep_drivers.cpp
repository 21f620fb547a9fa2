// r2l_lockstep_drivers.cpp -- the stand-alone drivers of the lock-step emulation as ONE program (own main, no Python): the
// emulation's sources (r2l_lockstep.cpp, unchanged: every kernel in its device form, the device's host route) compiled once with
// -fsanitize=address,undefined, and behind them the drivers, each a file and a namespace of its own with one
// `int run(int argc, char** argv)` (argv[0]: its name).  TEST INFRASTRUCTURE: built and run by tests/lockstep_driver.py.
// One process runs one driver: what a driver sets for itself (R2L_* overrides in the environment, the launch observer of
// r2l_lockstep_rt.h, the launch record) is never seen by another.
//   usage: r2l_lockstep_drivers <subcommand> [arguments]
#define R2L_TEST_HOOKS 1
#include "r2l_lockstep.cpp"

#include "r2l_driver_util.h"

#include "r2l_bn_settings_lockstep.cpp"
#include "r2l_channels_last_lockstep.cpp"
#include "r2l_fwd_routes_lockstep.cpp"
#include "r2l_half_io_lockstep.cpp"
#include "r2l_limits_lockstep.cpp"
#include "r2l_static_half_lockstep.cpp"
#include "r2l_static_routes_lockstep.cpp"
#include "r2l_entries_lockstep.cpp"  // (behind fwd_routes: it uses that driver's parameter block)

int main(int argc, char** argv) {
  static const struct {
    const char *name, *arguments;
    int (*run)(int, char**);
  } DRIVERS[8] = {{"half_io", " <params.bin>", r2l_drv::half_io::run}, {"channels_last", " <params.bin>", r2l_drv::channels_last::run},
                  {"static_half", "", r2l_drv::static_half::run},      {"static_routes", "", r2l_drv::static_routes::run},
                  {"fwd_routes", "", r2l_drv::fwd_routes::run},        {"limits", "", r2l_drv::limits::run},
                  {"bn_settings", "", r2l_drv::bn_settings::run},      {"entries", "", r2l_drv::entries::run}};
  for (const auto& d : DRIVERS)
    if (argc >= 2 && !strcmp(argv[1], d.name)) return d.run(argc - 1, argv + 1);
  fprintf(stderr, "usage: r2l_lockstep_drivers <subcommand> [arguments], the subcommands:\n");
  for (const auto& d : DRIVERS) fprintf(stderr, "  %s%s\n", d.name, d.arguments);
  return 2;
}
