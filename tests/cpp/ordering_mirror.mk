# C++ host-mirror test of the orderings: plain g++, links the C ABI only (make -f ordering_mirror.mk)
CXX ?= g++
ordering_mirror_test.bin: ordering_mirror_test.cpp ../../include/sprs_hip.hpp ../../include/sprs_hip.h
	$(CXX) -O2 -std=c++17 -Wall -o $@ ordering_mirror_test.cpp -L../../sprs_amd -lsprs_hip \
	    -Wl,-rpath,'$$ORIGIN/../../sprs_amd' -Wl,--allow-shlib-undefined
