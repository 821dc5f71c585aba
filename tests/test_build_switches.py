"""A compile-time switch stays in csrc/ only while something committed builds
its other side, and tools/README.md "Build switches" says what does.  The
sources are checked as text: every NAME with `#ifndef NAME` directly followed
by `#define NAME ...` is a switch, and the table lists exactly those."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "nydus-snapshotter_amd", "csrc")


def source_switches():
    names = set()
    for d, _, files in os.walk(CSRC):
        for f in files:
            text = open(os.path.join(d, f), errors="replace").read()
            names |= set(re.findall(r"^[ \t]*#[ \t]*ifndef[ \t]+(\w+)[ \t]*\n"
                                    r"[ \t]*#[ \t]*define[ \t]+\1\b", text, re.M))
    return names


def table_switches():
    readme = open(os.path.join(ROOT, "tools", "README.md")).read()
    section = readme.split("**Build switches**", 1)[1]
    rows = re.match(r"[^|]*((?:\|.*\n)+)", section).group(1).splitlines()
    assert rows[0].split("|")[1].strip() == "switch" and set(rows[1]) <= set("|- "), rows[:2]
    return {re.fullmatch(r"`(\w+)`", r.split("|")[1].strip()).group(1) for r in rows[2:]}


def test_build_switches_table_lists_every_switch_of_the_sources():
    assert source_switches() == table_switches() == {"B3_PRIO", "NGPU_DIAG_NOLOAD"}
