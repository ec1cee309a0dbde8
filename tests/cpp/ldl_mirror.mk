# C++ host-mirror test of the LDL^T path: plain g++, links the C ABI only (make -f ldl_mirror.mk)
CXX ?= g++
ldl_mirror_test.bin: ldl_mirror_test.cpp ../../include/sprs_hip.hpp ../../include/sprs_hip.h
	$(CXX) -O2 -std=c++17 -Wall -o $@ ldl_mirror_test.cpp -L../../sprs_amd -lsprs_hip \
	    -Wl,-rpath,'$$ORIGIN/../../sprs_amd' -Wl,--allow-shlib-undefined
