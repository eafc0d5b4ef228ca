"""The argument parser of `kmerust` without a device and without the binary: krust_amd/host/cli_args.h and the commands' parse_*_args
of kmerust_host.h through the stand-alone check program tests/cli_args_check.cpp (its own main, nothing preloaded), plain and under
ASan + UBSan -- as tests/test_clip_host.py drives tests/clip_host_check.cpp; and the shape the parser is meant to keep: one loop, every
list of accepted values written once, and no parse_*_args that prints or exits."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "krust_amd", "host")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]], ids=["plain", "asan-ubsan"])
def test_every_commands_parser(tmp_path, flags):
    exe = str(tmp_path / "cli_args_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, os.path.join(ROOT, "tests", "cli_args_check.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:exitcode=97", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    assert p.returncode == 0 and "cli_args_check ok" in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stdout + p.stderr


def test_the_parser_header_stands_alone(tmp_path):
    """cli_args.h needs nothing of the host layer: a program that includes it alone compiles."""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "%s"\nint main() { uint64_t v = 0; return kmerust::parse_u64("7", "N", 9, &v).empty() && v == 7 ? 0 : 1; }\n' % os.path.join(HOST, "cli_args.h"))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", str(tmp_path / "alone"), str(src)], check=True)
    assert subprocess.run([str(tmp_path / "alone")]).returncode == 0


def test_one_loop_and_every_list_once():
    cli, header, args = _read("krust_amd", "host", "kmerust.cpp"), _read("krust_amd", "host", "kmerust_host.h"), _read("krust_amd", "host", "cli_args.h")
    assert "value_of" not in cli + header + args
    assert len(re.findall(r"\.substr\(0, 2\)", cli + header + args)) == 1 and ".substr(0, 2)" in args      # the `key =` line
    assert len(re.findall(r"leak_at_exit\(\) =", cli)) == 1 and len(re.findall(r"catch \(const Error &e\)", cli)) == 4   # run_guarded, query's loader, __parse, --save
    assert len(re.findall(r"define KMERUST_UNDER_ASAN", cli)) == 1
    assert (cli + header + args).count('[possible values: "') == 1 and '[possible values: "' in args          # the one place that makes the text
    assert cli.count("[possible values: ") == 2                                                               # the two lines of --help
    for words in ('"fasta", "tsv", "json", "histogram"', '"auto", "fasta", "fastq"', '"summary", "profile"', '"summary", "tsv", "json"', '"fasta", "summary"',
                  '"gfa", "summary"', '"min", "max", "sum", "left", "right"', '"intersect", "union", "subtract", "count-subtract"'):
        assert (cli + header + args).count(words) == 1, words
    assert len(re.findall(r"invalid digit found in string", cli + header + args)) == 1


def test_no_parser_prints_or_exits():
    header, args = _read("krust_amd", "host", "kmerust_host.h"), _read("krust_amd", "host", "cli_args.h")
    assert not re.search(r"\b(exit|_exit|abort|printf|fprintf|fputs|puts|perror)\s*\(|std::c(out|err)", args)
    section = header[header.index("// What the arguments of each command say"):]          # every parser is defined behind this line
    assert set(re.findall(r"^inline \w+ (parse_\w+_args)\([^;]*\) \{", section, flags=re.M)) == {
        "parse_count_args", "parse_query_sequences_args", "parse_filter_args", "parse_two_index_args", "parse_compare_args", "parse_combine_args",
        "parse_index_args", "parse_graph_args", "parse_unitigs_args", "parse_gfa_args", "parse_clip_args"}
    assert not re.search(r"\b(exit|_exit|abort|printf|fprintf|fputs|puts|perror)\s*\(|std::c(out|err)|stderr|stdout", section)
