"""fastANI --tree --treeSupport B [--treeSupportSeed s]: the .support and .support.newick files of the three tree methods on the two
species of test_tree.tree_genomes, against a Python mirror over the same genomes — Sketch.boot_begin / boot_take, boot_identity,
Engine.tree_average / tree_nj / tree_single and Engine.tree_support_bootstrap — with -o, .matrix and .newick equal to the run without
the option, through --refSketch, -t 3 and --treeFill sketch, and the refusals by their text.  CPU: the tests/emu build of the library
and of the command line at 30 000 bases; GPU (-m gpu): the product library and fastani_amd/fastANI at 200 000."""
import os
import re
import subprocess

import numpy as np
import pytest

import orc
from fastani_amd.api import Sketch, boot_identity
from test_cluster import make_rows
from test_tree import EMU, ROOT, tree_genomes
from test_tree_support import leaf_sets, tree_of

B, SEED = 20, 7
SPECIES = (list(range(0, 6)), [6, 7, 8])                    # positions in the list of tree_genomes


def run(binary, args, ok=True, env=None):
    r = subprocess.run([binary] + args, capture_output=True, env=dict(os.environ, **(env or {})))
    assert (r.returncode == 0) == ok, r.stderr.decode()[-2000:]
    return r.stderr.decode()


def read_support(path):
    lines = open(path).read().splitlines()
    head = lines[0].split("\t")
    rec = [ln.split("\t") for ln in lines[1:]]
    assert [int(x[0]) for x in rec] == list(range(len(rec)))
    return head, rec


def strip_labels(text):
    """the percentages after a closing bracket, and the tree without them"""
    return re.findall(r"\)(\d+)", text), re.sub(r"\)\d+", ")", text)


def percent(support, replicates):
    return (200 * support + replicates) // (2 * replicates)


def check_files(out, names, method, replicates, seed):
    """what the two files hold by themselves: the header, the record form, the labels"""
    head, rec = read_support(out + ".support")
    assert head == ["#replicates", str(replicates), "seed", str(seed), "method", method]
    n = len(names)
    assert len(rec) == n - 1
    idx = dict((x, i) for i, x in enumerate(names))
    children = np.array([[idx[c] if not c.startswith("#") else n + int(c[1:]) for c in x[1:3]] for x in rec], dtype=np.int32)
    sets = leaf_sets(children, n)
    assert [int(x[3]) for x in rec] == [len(sets[n + s]) for s in range(n - 1)]
    support = [int(x[4]) for x in rec]
    assert all(0 <= v <= replicates for v in support)
    text, plain = open(out + ".support.newick").read(), open(out + ".newick").read()
    labels, stripped = strip_labels(text)
    assert stripped == plain
    # every closing bracket before the final one has a label; the final one has none
    bare = re.sub(r"'(?:[^']|'')*'", "Q", plain)             # (two of the names hold brackets of their own, in quotes)
    assert len(labels) == bare.count(")") - 1 and plain.rstrip().endswith(");") and not re.search(r"\)\d+;", text)
    # the labels are the percentages of the records, each clade's where the tree closes it: read the leaves between the brackets
    by_clade = {}
    for s in range(n - 1):
        c = sets[n + s]
        by_clade[c] = percent(support[s], replicates)
    stack, i, seen = [], 0, 0
    quoted = dict(("'%s'" % x.replace("'", "''"), i) for x, i in idx.items())
    while i < len(text):
        if text[i] == "(":
            stack.append(set())
            i += 1
        elif text[i] == ")":
            done = stack.pop()
            m = re.match(r"\d+", text[i + 1:])
            if stack:
                stack[-1] |= done
                assert m and int(m.group()) == by_clade[frozenset(done)], (sorted(done), m and m.group(), by_clade[frozenset(done)])
                seen += 1
            i += 1 + (len(m.group()) if m else 0)
        elif text[i] in ",;\n":
            i += 1
        elif text[i] == ":":
            i = re.compile(r"[,);]").search(text, i).start()
        else:
            if text[i] == "'":
                j = i + 1
                while True:
                    j = text.index("'", j)
                    if text[j + 1:j + 2] == "'":
                        j += 2
                        continue
                    break
                name = quoted[text[i:j + 1]]
                i = j + 1
            else:
                j = re.compile(r"[:,)]").search(text, i).start()
                name = idx[text[i:j]]
                i = j
            stack[-1].add(name)
    assert seen == len(labels)
    return children, support, sets


_mapped = {}


def mirror(engine, n_len, out_lines, paths, method, replicates, seed):
    """the same through the Python interface: the rows and replicate identities of the -o file's lines, in its order"""
    key = (id(engine), n_len, replicates, seed)
    if key not in _mapped:                                  # (one mapping for the three methods)
        genomes = [[orc.synth_genome(17, g, n_len)] for g in list(range(0, 6)) + [20, 21, 22]]
        sk = Sketch(engine, engine.params(16, 3000), genomes)
        sk.boot_begin(replicates=replicates, seed=seed)
        rows = sk.map_cgi_batch(genomes, 0)
        _mapped.clear()
        _mapped[key] = (rows,) + sk.boot_take()
        sk.boot_end()
        sk.close()
    rows, rec, sums = _mapped[key]
    assert len(rec) == len(rows) and np.array_equal(rec["refGenomeId"], rows["refGenomeId"]) and np.array_equal(rec["qryGenomeId"], rows["qryGenomeId"])
    rep = boot_identity(rec, sums)
    at = dict(((int(r["qryGenomeId"]), int(r["refGenomeId"])), i) for i, r in enumerate(rows))
    idx = dict((p, i) for i, p in enumerate(paths))
    keep = []
    for line in out_lines:
        q, r = line.split("\t")[:2]
        if q != r:
            keep.append(at[(idx[q], idx[r])])
    assert len(keep) >= 30
    rows, rep = rows[keep], np.ascontiguousarray(rep[keep])
    assert (rep.min(axis=1) < rep.max(axis=1)).any()
    tree_rows = make_rows([(int(min(q, r)), int(max(q, r)), x) for q, r, x in zip(rows["qryGenomeId"], rows["refGenomeId"], rows["identity"])])
    children = tree_of(engine, method, tree_rows, len(paths))
    return children, engine.tree_support_bootstrap(method, tree_rows, len(paths), rep, children)


def run_cli(binary, engine, tmp, n_len):
    lst = tree_genomes(tmp, n_len)
    paths = open(lst).read().rstrip("\n").split("\n")
    common = ["--ql", lst, "--rl", lst, "--matrix", "--tree"]
    for method in ("average", "nj", "single"):
        plain, out = os.path.join(tmp, "plain_%s.out" % method), os.path.join(tmp, "s_%s.out" % method)
        run(binary, common + ["--treeMethod", method, "-o", plain])
        assert not os.path.exists(plain + ".support") and not os.path.exists(plain + ".support.newick")
        run(binary, common + ["--treeMethod", method, "--treeSupport", str(B), "--treeSupportSeed", str(SEED), "-o", out])
        suffixes = sorted(f[len("plain_%s.out" % method):] for f in os.listdir(tmp) if f.startswith("plain_%s.out" % method))
        assert sorted(f[len("s_%s.out" % method):] for f in os.listdir(tmp) if f.startswith("s_%s.out" % method)) == sorted(suffixes + [".support", ".support.newick"])
        for suffix in suffixes:                             # -o, .matrix, .newick (and .mst): byte for byte
            assert open(plain + suffix, "rb").read() == open(out + suffix, "rb").read(), (method, suffix)
        children, support, sets = check_files(out, paths, method, B, SEED)
        # the clade that splits the two species: every replicate
        at = dict((sets[len(paths) + s], s) for s in range(len(paths) - 1))
        split = [c for c in (frozenset(SPECIES[0]), frozenset(SPECIES[1])) if c in at]
        assert split and all(support[at[c]] == B for c in split), (method, support)
        m_children, m_support = mirror(engine, n_len, open(out).read().splitlines(), paths, method, B, SEED)
        assert m_children.tolist() == children.tolist() and m_support.tolist() == support, (method, m_support.tolist(), support)
        # the default seed is 1, and another seed is another file header
        if method == "average":
            one = os.path.join(tmp, "seed1.out")
            run(binary, common + ["--treeSupport", "3", "-o", one])
            assert read_support(one + ".support")[0] == ["#replicates", "3", "seed", "1", "method", "average"]
        # the same files through the other paths of the command line
        ref = dict((s, open(out + s, "rb").read()) for s in (".support", ".support.newick", ".newick"))
        sketch = os.path.join(tmp, "refs_%s.anisk" % method)
        opts = ["--treeMethod", method, "--treeSupport", str(B), "--treeSupportSeed", str(SEED)]
        for name, args in (("save", ["--ql", lst, "--rl", lst, "--saveSketch", sketch]), ("sketch", ["--ql", lst, "--refSketch", sketch]),
                           ("threads", ["--ql", lst, "--rl", lst, "-t", "3", "--matrix"])):
            o = os.path.join(tmp, "v_%s_%s.out" % (name, method))
            run(binary, args + ["--tree"] + opts + ["-o", o])
            for s in ref:
                assert open(o + s, "rb").read() == ref[s], (method, name, s)
        # --treeFill sketch: fill cells do not vary; the files agree with each other and with the run without the option, and
        # the streamed single-linkage path steps aside for the pair step's below its ceiling
        fill_plain, fill = os.path.join(tmp, "fp_%s.out" % method), os.path.join(tmp, "f_%s.out" % method)
        run(binary, common + ["--treeMethod", method, "--treeFill", "sketch", "-o", fill_plain])
        run(binary, common + opts + ["--treeFill", "sketch", "-o", fill])
        assert open(fill + ".newick", "rb").read() == open(fill_plain + ".newick", "rb").read()
        f_children, f_support, f_sets = check_files(fill, paths, method, B, SEED)
        f_at = dict((f_sets[len(paths) + s], s) for s in range(len(paths) - 1))
        assert all(f_support[f_at[c]] == B for c in (frozenset(SPECIES[0]), frozenset(SPECIES[1])) if c in f_at)
        if method == "single":
            streamed = os.path.join(tmp, "fs_single.out")
            run(binary, common + opts + ["--treeFill", "sketch", "-o", streamed], env=dict(ANI_TEST_CLI_SINGLE_STREAM="1"))
            for s in (".support", ".support.newick", ".newick", ".mst"):
                assert open(streamed + s, "rb").read() == open(fill + s, "rb").read(), s
    # the refusals, before anything is mapped
    refused = os.path.join(tmp, "refused.out")
    for args, msg in ((["--ql", lst, "--rl", lst, "--treeSupport", "10"], "ERROR, --treeSupport needs --tree"),
                      (common + ["--treeSupportSeed", "3"], "ERROR, --treeSupportSeed needs --treeSupport"),
                      (common + ["--treeSupport", "0"], "ERROR, --treeSupport takes a replicate count in 1 .. 1024"),
                      (common + ["--treeSupport", "1025"], "ERROR, --treeSupport takes a replicate count in 1 .. 1024"),
                      (common + ["--treeSupport", "-3"], "ERROR, --treeSupport takes a replicate count in 1 .. 1024"),
                      (common + ["--treeSupport", "ten"], "ERROR, --treeSupport takes a replicate count in 1 .. 1024")):
        assert msg in run(binary, args + ["-o", refused], ok=False), args
    # the streamed single-linkage path beyond 65 536 genomes: refused on the list alone — 65 537 spellings of one file's path
    big = os.path.join(tmp, "big.txt")
    open(big, "w").write("".join("%s/%st0.fa\n" % (tmp, "".join(".//" if i >> k & 1 else "./" for k in range(17))) for i in range(65537)))
    err = run(binary, ["--ql", big, "--rl", big, "--tree", "--treeMethod", "single", "--treeFill", "sketch", "--treeSupport", "10", "-o", refused], ok=False)
    assert "ERROR, --treeSupport takes at most 65536 genomes" in err
    assert not os.path.exists(refused)


def test_cli_tree_support_cpu_build(emu_engine, tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU, "all"])
    run_cli(os.path.join(EMU, "fastANI_emu"), emu_engine, str(tmp_path), 30000)


@pytest.mark.gpu
def test_cli_tree_support_gpu(gpu_engine, tmp_path):
    binary = os.path.join(ROOT, "fastani_amd", "fastANI")
    assert os.path.exists(binary), "build the CLI with __graft_entry__.build()"
    run_cli(binary, gpu_engine, str(tmp_path), 200000)
