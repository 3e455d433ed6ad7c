"""The worklist kernels fold through one layer (worklist.hip.h: wl_wave_fold, wl_block_fold, wl_block_part, wl_sum_parts,
wl_from_thread0, wl_jump): the per-algorithm copies are gone from csrc/, and what is left of wave shuffles and per-wave or
per-thread LDS words in the graph headers is the short list below, each entry with the reason why it is no fold.  Source
checks only (no GPU needed)."""
import os
import re

from abi_checks import CSRC

REMOVED = ("wcc_block_part", "scc_block_part", "gcol_block_part", "truss_block_part", "truss_sum_parts", "truss_wave_sum64",
           "core_block_min", "tri_block_sums", "gcol_wave_sync", "tri_wave_sync", "gcol_load", "truss_load", "scc_umax",
           "sssp_umax")
GRAPH_HEADERS = ("bfs", "sssp", "scc", "wcc", "tri", "core", "truss", "color", "msf", "match", "rcm", "frontier")
CLOSING = {"bfs": "bfs_decide", "sssp": "sssp_decide", "scc": "scc_decide", "wcc": "wcc_decide", "core": "core_close",
           "truss": "truss_close", "color": "gcol_close", "msf": "msf_close", "match": "match_close", "rcm": "rcm_close"}
# (header, function) -> why its shuffles or LDS words are not a fold of the layer's
EXCEPTIONS = {
    ("rcm", "rcm_block_scan"): "an exclusive prefix over the workgroup's threads: a scan, every thread gets another word",
    ("rcm", "rcm_tile"): "ranks the chosen entries of a list (per-wave counts before this wave) and queues the long lists",
    ("sssp", "sssp_weight_sum"): "adds doubles: another order changes the default delta's last bits and exact round counts",
    ("frontier", "fr_wave_reduce"): "typed by the semiring, whose add is no integer sum, min or max",
    ("frontier", "frontier_detect"): "the compaction: a workgroup's waves reserve consecutive places, a scan of four counts",
    ("scc", "scc_block_best"): "an arg-max over a (64-bit product, vertex) pair, which fits no word the layer folds",
    ("tri", "tri_count_heavy"): "s_todo[WL_BS] is a list of rows the workgroup takes one by one, nothing is folded",
}
SHUFFLE = re.compile(r"__shfl_xor")
WORDS = re.compile(r"__shared__[^;]*\[WL_BS(?: / 64)?\](?!\[)")   # (a [WL_BS / 64][n] array is n words per wave: staging)
DEFINITION = re.compile(r"^(?:__global__|__device__)(?: __launch_bounds__\(\w+\))?[^;(]*?(\w+)\(")


def read(name):
    return open(os.path.join(CSRC, name)).read()


def occurrences(header):
    """-> the functions of `header`.hip.h that hold a shuffle-xor or a 1-D LDS array of WL_BS / 64 or WL_BS words"""
    found, fn = set(), None
    for line in read(header + ".hip.h").splitlines():
        m = DEFINITION.match(line)
        if m:
            fn = m.group(1)
        if SHUFFLE.search(line.split("//")[0]) or WORDS.search(line.split("//")[0]):
            found.add((header, fn))
    return found


def test_the_copies_are_gone_from_csrc():
    for name in sorted(os.listdir(CSRC)):
        if os.path.isfile(os.path.join(CSRC, name)):
            text = read(name)
            for word in REMOVED:
                assert not re.search(r"\b" + word + r"\b", text), (name, word)


def test_shuffles_and_fold_words_stand_in_the_listed_exceptions_only():
    found = set()
    for header in GRAPH_HEADERS:
        found |= occurrences(header)
    assert found == set(EXCEPTIONS), (sorted(found - set(EXCEPTIONS)), sorted(set(EXCEPTIONS) - found))
    assert all(len(why) > 20 for why in EXCEPTIONS.values())
    # the finder finds: the layer itself holds the shuffle and the per-wave words
    layer = occurrences("worklist")
    assert layer == {("worklist", "wl_wave_fold"), ("worklist", "wl_block_fold"), ("worklist", "wl_block_fold_part")}, layer


def test_the_layer_states_its_contract_and_the_closing_kernels_gate_through_it():
    layer = read("worklist.hip.h")
    fold = layer[layer.index("// The workgroup's word -> EVERY thread"):layer.index("wl_from_thread0")]
    for phrase in ("CONVERGENT CONTROL FLOW ONLY", "EVERY thread", "as often as it", "__shared__ T s_w[WL_BS / 64];"):
        assert phrase in fold, phrase
    body = fold[fold.index("__shared__ T s_w"):]
    first_barrier, first_store = body.index("__syncthreads();"), body.index("s_w[threadIdx.x >> 6] = v;")
    assert first_barrier < first_store and body.count("__syncthreads();") == 2   # the barrier ahead of the words
    # the fold of a part has one barrier and none ahead of its words: it says so, its words are its own, the part writer
    # and the part fold are its only callers, and no kernel calls them twice on one path
    contract = layer[layer.index("// The workgroup's WlPart -> EVERY thread"):layer.index("struct WlNone")]
    for phrase in ("CONVERGENT CONTROL FLOW ONLY", "ONCE PER KERNEL", "none ahead of them"):
        assert phrase in contract, phrase
    part = layer[layer.index("wl_block_fold_part(uint32_t a"):layer.index("// The workgroup's words -> its WlPart")]
    assert part.count("__syncthreads();") == 1 and "__shared__ uint32_t s_w[HAS_C ? 3 : 2][WL_BS / 64];" in part
    for user in ("void wl_block_part(", "WlPart wl_sum_parts("):   # the one part writer and the one part fold
        body = layer[layer.index(user):]
        assert "wl_block_fold_part<OPB, OPC>(a, b, c)" in body[:body.index("\n}\n")], user
    assert layer.count("wl_block_fold_part<") == 2
    for header in GRAPH_HEADERS:
        text = read(header + ".hip.h")
        assert "wl_block_fold_part" not in text, header
        for kernel in re.split(r"\n(?=__global__ )", text)[1:]:
            name = DEFINITION.match(kernel).group(1)
            calls = len(re.findall(r"\bwl_(?:block_part|sum_parts)\b", kernel[:kernel.index("\n}\n")]))
            if name == "scc_trim":   # its two phases are two launches: phase 0 returns behind its part, phase 1 writes the other
                first = kernel.index("wl_block_part(")
                assert calls == 2 and re.match(r"wl_block_part\([^;]*;\s*return;", kernel[first:]), name
            else:
                assert calls <= 1, name
    gate = layer[layer.index("// A word of thread 0"):layer.index("wl_from_thread0(uint32_t v) {")]
    for phrase in ("one LDS word, one barrier", "thread 0 stores the next step", "leave before a barrier"):
        assert phrase in " ".join(gate.replace("//", " ").split()), phrase
    for header, kernel in CLOSING.items():
        text = read(header + ".hip.h")
        body = text[text.index("void " + kernel + "("):]
        body = body[:body.index("\n}\n")]
        assert body.count("wl_from_thread0(") == 1 and "s_go" not in text, kernel
    for header, limit in (("wcc", "WCC_JUMPS"), ("msf", "MSF_JUMPS")):
        text = read(header + ".hip.h")
        assert "wl_jump(i, " + limit + ", rows, p, jpart, ctl->moved);" in text
        assert "p[v] = q = up" not in text   # the body is the layer's
        assert "roots = wl_block_fold<WlSum>(roots);" in text
    for name in ("wl_wave_sync", "wl_load", "wl_umax", "wl_umin", "wl_jump", "struct WlSum", "struct WlMin", "struct WlMax"):
        assert name in layer, name
    for name in ("msf_lower", "msf_load"):
        assert name in read("msf.hip.h")
    assert "scc_cas" in read("scc.hip.h")


def test_truss_no_longer_borrows_from_core():
    includes = re.findall(r'^#include "([^"]+)"(.*)$', read("truss.hip.h"), re.M)
    assert [name for name, _ in includes] == ["worklist.hip.h"], includes
