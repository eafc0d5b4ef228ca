// cli_args.h -- the argument parser of the `kmerust` command line: a command is a table of options and a list of positionals, and one
// loop walks the arguments.  Pure and header-only: no device, no library call, no exit and no printing -- a refusal comes back as the
// text of the usage error (what follows "error: "), the first one in argv order.  The commands' tables are in kmerust_host.h
// (parse_*_args); tests/cli_args_check.cpp runs them stand-alone.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace kmerust {

// The accepted spellings of an enumerated value.  A value is stored as its position in the list, and the "[possible values: ...]"
// text is made from the same list.
using Choices = std::vector<const char *>;

// A validator for a value that is neither a number nor one of a list: stores v's meaning in *to, or returns the whole usage error.
// `what` is the option as messages name it: "--min-fraction <F>".
using Check = std::string (*)(const std::string &v, const std::string &what, void *to);

inline std::string invalid_value(const std::string &v, const std::string &what, const std::string &why) {
    return "invalid value '" + v + "' for '" + what + "'" + why;
}

// Decimal digits only (no sign, no blanks), at most 20 of them, a value of at most `max`.
inline std::string parse_u64(const std::string &s, const std::string &what, uint64_t max, uint64_t *v) {
    if (s.empty() || s.find_first_not_of("0123456789") != std::string::npos || s.size() > 20)
        return invalid_value(s, what, ": invalid digit found in string");
    uint64_t x = 0;
    for (char ch : s) {
        const uint64_t d = (uint64_t)(ch - '0');
        if (x > (UINT64_MAX - d) / 10) return invalid_value(s, what, ": number too large to fit in target type");
        x = x * 10 + d;
    }
    if (x > max) return invalid_value(s, what, ": number too large to fit in target type");
    *v = x;
    return "";
}

inline std::string parse_choice(const std::string &s, const std::string &what, const Choices &values, size_t *v) {
    std::string list;
    for (size_t i = 0; i < values.size(); ++i) {
        if (s == values[i]) {
            *v = i;
            return "";
        }
        list += std::string(i ? ", " : "") + values[i];
    }
    return invalid_value(s, what, "\n  [possible values: " + list + "]");
}

// One option.  A flag (value_name == nullptr) matches the whole argument: "--sorted=1" is not "--sorted".  A valued option matches the
// key -- the text before '=' of a "--" argument, the first two characters of any other -- and takes "--opt=v", "--opt v", "-o v" or
// "-ov".  Exactly one of the targets is set; make one with flag() ... custom().
struct Opt {
    const char *short_key, *long_key;  // "-f", "--format"; short_key may be nullptr
    const char *value_name;            // "<FORMAT>"
    bool *flag;
    bool stops;                        // a flag that ends the walk at once (--help)
    uint64_t *number;
    uint64_t max;
    const Choices *values;
    size_t *choice;
    std::string *text;
    Check check;
    void *to;
    bool *seen;                        // (optional) set when the option's value was taken
};
inline Opt flag(const char *s, const char *l, bool *to, bool stops = false) { return {s, l, nullptr, to, stops, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; }
inline Opt number(const char *s, const char *l, const char *name, uint64_t *to, uint64_t max = UINT64_MAX, bool *seen = nullptr) {
    return {s, l, name, nullptr, false, to, max, nullptr, nullptr, nullptr, nullptr, nullptr, seen};
}
inline Opt choice(const char *s, const char *l, const char *name, const Choices &values, size_t *to) {
    return {s, l, name, nullptr, false, nullptr, 0, &values, to, nullptr, nullptr, nullptr, nullptr};
}
inline Opt text(const char *s, const char *l, const char *name, std::string *to, bool *seen = nullptr) {
    return {s, l, name, nullptr, false, nullptr, 0, nullptr, nullptr, to, nullptr, nullptr, seen};
}
inline Opt custom(const char *s, const char *l, const char *name, Check check, void *to) {
    return {s, l, name, nullptr, false, nullptr, 0, nullptr, nullptr, nullptr, check, to, nullptr};
}

struct Command {
    std::vector<Opt> opts;
    std::vector<const char *> positionals;  // their names in order: "<INDEX>"; the walk takes no more than these
    size_t required;                        // how many of them have to be there
    const char *usage;                      // "Usage: kmerust graph <INDEX>"
};

// Walks args: options into their targets, everything else into *pos.  A lone "-" is a positional; any other argument that starts
// with '-' and is no option of the command is unexpected.  Returns "" or the first usage error.
inline std::string parse_args(const Command &cmd, const std::vector<std::string> &args, std::vector<std::string> *pos) {
    for (size_t i = 0; i < args.size(); ++i) {
        const std::string &a = args[i];
        const bool dashes = a.rfind("--", 0) == 0;
        const size_t eq = a.find('=');
        const std::string key = dashes ? a.substr(0, eq) : a.substr(0, 2);
        const Opt *o = nullptr;
        for (const Opt &c : cmd.opts) {
            const std::string &m = c.value_name ? key : a;
            if ((c.short_key && m == c.short_key) || m == c.long_key) {
                o = &c;
                break;
            }
        }
        if (!o) {
            if ((a.size() > 1 && a[0] == '-') || pos->size() == cmd.positionals.size()) return "unexpected argument '" + a + "' found";
            pos->push_back(a);
            continue;
        }
        if (!o->value_name) {
            *o->flag = true;
            if (o->stops) return "";
            continue;
        }
        const std::string what = std::string(o->long_key) + " " + o->value_name;
        std::string v, err;
        if (dashes && eq != std::string::npos) v = a.substr(eq + 1);
        else if (!dashes && a.size() > 2) v = a.substr(2);  // -fVALUE
        else if (i + 1 >= args.size()) return "a value is required for '" + what + "' but none was supplied";
        else v = args[++i];
        if (o->number) err = parse_u64(v, what, o->max, o->number);
        else if (o->choice) err = parse_choice(v, what, *o->values, o->choice);
        else if (o->text) *o->text = v;
        else err = o->check(v, what, o->to);
        if (!err.empty()) return err;
        if (o->seen) *o->seen = true;
    }
    return "";
}

// The refusal of a command line without all of its required positionals, or "".
inline std::string missing_args(const Command &cmd, const std::vector<std::string> &pos) {
    if (pos.size() >= cmd.required) return "";
    std::string msg = "the following required arguments were not provided:";
    for (size_t j = pos.size(); j < cmd.required; ++j) msg += std::string("\n  ") + cmd.positionals[j];
    return msg + "\n\n" + cmd.usage;
}

}  // namespace kmerust
