# Stand-alone sanitizer run of the host-side argument checks of the dense <-> sparse entries: the library's sources compiled for
# the HOST with the headers of tests/emu (no device code, no device needed) under AddressSanitizer and UBSan, linked into one
# program with its own main.  `make -f dense_args_asan.mk dense_args_asan.bin && ./dense_args_asan.bin` (tests/test_dense_asan_cpu.py does that).
HOSTCXX := /opt/rocm/lib/llvm/bin/clang++
CSRC := ../../sprs_amd/csrc
ASAN_SRCS := abi spmv spmv_band spgemm scan convert spmm bicgstab gauss_seidel sort triplet dist
ASAN_FLAGS := -std=c++17 -O0 -g -fPIC -ffp-contract=off -I../emu -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -fno-omit-frame-pointer -Wno-unused-result -Wno-unknown-attributes -Wno-unused-value

asan_obj/%.o: $(CSRC)/%.hip
	@mkdir -p asan_obj
	$(HOSTCXX) -x c++ $(ASAN_FLAGS) -MMD -MP -c $< -o $@

asan_obj/hipemu.o: ../emu/hipemu.cpp ../emu/hip/hip_runtime.h
	@mkdir -p asan_obj
	$(HOSTCXX) $(ASAN_FLAGS) -c $< -o $@

asan_obj/dense_args_asan.o: dense_args_asan.cpp ../../include/sprs_hip.h
	@mkdir -p asan_obj
	$(HOSTCXX) $(ASAN_FLAGS) -c $< -o $@

dense_args_asan.bin: $(ASAN_SRCS:%=asan_obj/%.o) asan_obj/hipemu.o asan_obj/dense_args_asan.o
	$(HOSTCXX) -fsanitize=address,undefined -o $@ $^ -ldl

-include $(ASAN_SRCS:%=asan_obj/%.d)
