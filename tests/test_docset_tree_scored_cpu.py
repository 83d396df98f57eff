"""The constants of scored doc sets of phrases and nested boolean queries (tantivy_amd/csrc/tq_docset_tree_score.hip,
option "docset_score_trees") in the binding: the TQ_KERNEL_DOCSET_TREE_SCORE bit of include/tantivy_amd.h and its name,
and the option's documentation.  No GPU needed."""
import os
import re

from tantivy_amd import binding as B
from tantivy_amd import build as product_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "tantivy_amd.h")) as f:
        return f.read()


def test_kernel_bit_and_name():
    assert B.KERNEL_DOCSET_TREE_SCORE == 0x20000
    assert B.kernel_names(B.KERNEL_DOCSET_TREE_SCORE) == ["docset_tree_score"]
    mask = B.KERNEL_DOCSET | B.KERNEL_DOCSET_SCORE | B.KERNEL_DOCSET_TREE | B.KERNEL_DOCSET_TREE_SCORE
    assert B.kernel_names(mask) == ["docset", "docset_score", "docset_tree", "docset_tree_score"]
    bits = list(B.KERNEL_NAMES)
    assert len(set(bits)) == len(bits) and all(b & (b - 1) == 0 for b in bits)  # one bit each


def test_header_define_and_option():
    header = _header()
    m = re.search(r"#define\s+TQ_KERNEL_DOCSET_TREE_SCORE\s+0x([0-9a-fA-F]+)u", header)
    assert m and int(m.group(1), 16) == B.KERNEL_DOCSET_TREE_SCORE
    assert '"docset_score_trees"' in header
    # the sentence that stays true: "docset_trees" concerns the unscored calls alone
    assert re.search(r'"docset_trees"\s*=\s*1,\s*which\s+only\s+concerns\s+the\s+unscored\s+calls', header)


def test_kernel_file_is_built_and_attributed():
    src = os.path.join(os.path.dirname(product_build.__file__), "csrc", "tq_docset_tree_score.hip")
    assert src in product_build.SOURCES and os.path.exists(src)
    assert product_build.KERNEL_FILES["docset_tree_score_kernel"] == "tq_docset_tree_score.hip"


def test_raw_search_trees_exists():
    assert callable(getattr(B.DeviceIndex, "raw_search_trees"))
