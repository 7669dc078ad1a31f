"""The batch resampler's tile kernels after they were composed from resample_steps.hpp: nothing spills, nothing goes to
scratch, and no kernel holds fewer wavefronts per SIMD than the kernel it replaced.  Compile only (hipcc cross-compiles
without a GPU), the flags of kernel_remarks.py."""
import pytest

import kernel_remarks

# Occupancy [waves/SIMD] of commit bf350d5's kernels, from the same compile: resample_up_kernel<3,48,8,false,false> (the
# benchmark's leg), resample_down_kernel<N,48,8> for N = 2, 3, 4, 6 -- now resample_split_kernel<1,N,48,8> -- and
# resample_ratio_kernel<3,2,24,8> / <2,3,24,8> -- now resample_split_kernel<3,2,24,8> / <2,3,24,8>
PARENT_OCCUPANCY = {
    "resample_up_kernelILi3ELi48ELi8ELb0ELb0EE": 4,
    "resample_split_kernelILi1ELi2ELi48ELi8EE": 4,
    "resample_split_kernelILi1ELi3ELi48ELi8EE": 4,
    "resample_split_kernelILi1ELi4ELi48ELi8EE": 4,
    "resample_split_kernelILi1ELi6ELi48ELi8EE": 4,
    "resample_split_kernelILi3ELi2ELi24ELi8EE": 4,
    "resample_split_kernelILi2ELi3ELi24ELi8EE": 4,
}


@pytest.fixture(scope="module")
def remarks():
    return kernel_remarks.remarks("resample.hip")


def test_the_split_kernel_has_these_instances_and_no_other(remarks):
    names = {n for n, _ in kernel_remarks.usages(remarks, "resample_split_kernel")}
    assert len(names) == 6 and all(any(k in n for n in names) for k in PARENT_OCCUPANCY if "split" in k), names
    assert not kernel_remarks.usages(remarks, "resample_down_kernel") and not kernel_remarks.usages(remarks, "resample_ratio_kernel")


@pytest.mark.parametrize("kernel", sorted(PARENT_OCCUPANCY))
def test_no_spill_no_scratch_and_the_parents_occupancy(remarks, kernel):
    found = kernel_remarks.usages(remarks, kernel)
    assert len(found) == 1, (kernel, [n for n, _ in found])
    name, u = found[0]
    assert int(u["VGPRs Spill"]) == 0, (name, u)
    assert int(u["ScratchSize [bytes/lane]"]) == 0, (name, u)
    assert int(u["Occupancy [waves/SIMD]"]) >= PARENT_OCCUPANCY[kernel], (name, u)
