// mps.h -- the commands of the `mps` host program, one translation unit each (cmd_<name>.cpp), and the phase timer they
// share.  Every command takes main's argv (argv[1] is its name), returns the exit status, throws Fatal for bad input and
// EngineError for a failed device call (mps_main.cpp turns both into a message and a status).
#pragma once
#include <chrono>
#include <cstdlib>
#include <iostream>

namespace host {

int cmd_cusk(int argc, char **argv);
int cmd_cuskss(int argc, char **argv);
int cmd_sumstats(int argc, char **argv);
int cmd_cuskss_bed(int argc, char **argv);
int cmd_block(int argc, char **argv);
int cmd_prune(int argc, char **argv);
int cmd_prep(int argc, char **argv);
int cmd_prep_phen(int argc, char **argv);
int cmd_check_phen(int argc, char **argv);

// wall-clock phase marks, printed as "[t] <phase>: <ms> ms" when CUSK_TIMING is set (tools/e2e_block.py)
struct PhaseTimer
{
    bool on = std::getenv("CUSK_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), last = t0;
    void mark(const char *what)
    {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        std::cout << "[t] " << what << ": " << std::chrono::duration<double, std::milli>(now - last).count() << " ms (at "
                  << std::chrono::duration<double, std::milli>(now - t0).count() << ")" << std::endl;
        last = now;
    }
};

}  // namespace host
