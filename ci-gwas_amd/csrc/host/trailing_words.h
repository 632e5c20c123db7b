// trailing_words.h -- the optional words behind the positional arguments of `mps cusk`, `mps sumstats` and
// `mps cuskss-bed` (het, filter, rows, markers, se, ordinal=...).  A command declares its words and where each may stand;
// one parser applies the rules and names the first argument that breaks them.  Pure host code
// (tools/square_inputs_selftest.cpp tabulates it).
#pragma once
#include <string>
#include <vector>

#include "host_io.h"

namespace host {

struct TrailingWord
{
    enum : int { kAnywhere = -1, kLast = -2, kFree = -3 };
    const char *name;   // a name that ends in '=' matches every argument that starts with it
    int at;             // the one place it may stand, counted from the first trailing argument; or kAnywhere, or kLast; or
                        // kFree: anywhere, and it needs no leading word in front of it
    bool *on;           // set when the word is given
    std::string *text;  // not NULL: receives the whole argument
};

// argv[first ..] against `words`.  words[0] is the leading word: without it nothing but a kFree word may follow, and it
// stands first.  Every word at most once.  Dies with "<cmd>: unknown trailing argument <arg>" (status 1) at the first argument that is no word
// of the command, is repeated, or stands where its word may not.
inline void parse_trailing_words(const char *cmd, int argc, char **argv, int first, const std::vector<TrailingWord> &words)
{
    for (const TrailingWord &w : words) *w.on = false;
    for (int a = first; a < argc; a++)
    {
        const std::string arg = argv[a];
        const TrailingWord *hit = nullptr;
        for (const TrailingWord &w : words)
        {
            const std::string name = w.name;
            const bool match = name.back() == '=' ? arg.compare(0, name.size(), name) == 0 : arg == name;
            const int place = a - first;
            const bool lead = &w == &words[0];
            const bool free_word = !lead && w.at == TrailingWord::kFree;
            if (match && !*w.on && (free_word || lead == (place == 0)) &&
                (lead || free_word || w.at == TrailingWord::kAnywhere || (w.at == TrailingWord::kLast ? a + 1 == argc : w.at == place)))
                hit = &w;
        }
        if (!hit) die(std::string(cmd) + ": unknown trailing argument " + argv[a]);
        *hit->on = true;
        if (hit->text) *hit->text = arg;
    }
}

}  // namespace host
