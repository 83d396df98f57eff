"""The constants of doc sets of phrases and nested boolean queries (tantivy_amd/csrc/tq_docset_tree.hip, option
"docset_trees") in the binding: the TQ_KERNEL_DOCSET_TREE bit of include/tantivy_amd.h and its name.  No GPU needed."""
import re
from pathlib import Path

from tantivy_amd import binding as B

ROOT = Path(__file__).resolve().parent.parent


def test_kernel_mask_bit_and_name():
    assert B.KERNEL_DOCSET_TREE == 0x10000
    assert B.kernel_names(B.KERNEL_DOCSET_TREE) == ["docset_tree"]
    names = B.kernel_names(B.KERNEL_DOCSET | B.KERNEL_DOCSET_TREE)
    assert "docset" in names and "docset_tree" in names and len(names) == 2


def test_the_header_defines_the_same_bit_and_documents_the_option():
    header = (ROOT / "include" / "tantivy_amd.h").read_text()
    m = re.search(r"#define\s+TQ_KERNEL_DOCSET_TREE\s+0x([0-9a-fA-F]+)u", header)
    assert m and int(m.group(1), 16) == B.KERNEL_DOCSET_TREE
    assert '"docset_trees"' in header
