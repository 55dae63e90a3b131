"""The code-object metadata of the device listings the build keeps (build/<stem>-hip-amdgcn-amd-amdhsa-gfx950.s), for the tests that
hold a source to its kernels and their register, scratch and LDS budgets.  Metadata only: no instruction of a listing is read."""
import os
import re


def parse_listing(txt):
    """The text of one listing -> {mangled kernel name: dict(vgpr, spill, sspill, scratch, lds, threads)}."""
    meta = {}
    for blk in re.findall(r"- \.agpr_count:.*?(?=\n  - \.agpr_count:|\namdhsa\.target)", txt, flags=re.S):
        get = lambda key: re.search(r"\.%s:\s+(\S+)" % key, blk).group(1)
        meta[get("name")] = dict(vgpr=int(get("vgpr_count")), spill=int(get("vgpr_spill_count")), sspill=int(get("sgpr_spill_count")),
                                 scratch=int(get("private_segment_fixed_size")), lds=int(get("group_segment_fixed_size")),
                                 threads=int(get("max_flat_workgroup_size")))
    return meta


def kernel_metadata(stem):
    """Build, then the kernels of csrc/<stem>.hip as ``parse_listing`` gives them."""
    import __graft_entry__ as g
    g.build()
    path = os.path.join(g.PKG, "build", "%s-hip-amdgcn-amd-amdhsa-gfx950.s" % stem)
    assert os.path.exists(path), "the build keeps the device listing of every source (csrc/Makefile, --save-temps=obj)"
    return parse_listing(open(path).read())
