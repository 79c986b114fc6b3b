"""lfamd_packed_size is the parent commit's (no GPU: the size is host arithmetic from the layout table of lfamd_internal.h): the
size column of tests/golden/pack_images_parent.json, at the shapes of the image cases and of test_abi_exports / test_pad256_abi."""
import pack_image_cases as pic


def test_packed_size_is_the_parents():
    from llamafile_amd import _hip
    L = pic.bind(_hip.HIP_SO)
    g = pic.golden()
    assert sorted(g["sizes"]) == sorted({pic.case_id(*c) for c in pic.size_only_cases()})
    for c in pic.size_only_cases():
        assert pic.packed_size(L, *c) == g["sizes"][pic.case_id(*c)], pic.case_id(*c)
    for c in pic.cases():
        assert pic.packed_size(L, *c) == g["cases"][pic.case_id(*c)]["size"] > 0, pic.case_id(*c)
