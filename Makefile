# Builds libtic.so (gfx950 HIP kernels + C-ABI runtime) in-tree so it travels with the
# repo snapshot to the GPU box.  `make -j8` here cross-compiles without a GPU.
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
CSRC     := tf_image_compression_amd/csrc
BUILD    := build
LIB      := tf_image_compression_amd/libtic.so
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Iinclude -I$(CSRC)
KERNELS  := conv_s1 conv_s2 conv_t2 conv_rgb conv_chain image_ops
OBJS     := $(addprefix $(BUILD)/,$(addsuffix .o,$(KERNELS))) $(BUILD)/tic_entropy_emb.o $(BUILD)/range_coder.o \
            $(BUILD)/host_util.o
HDRS     := $(wildcard $(CSRC)/*.h) include/tic.h

all: $(LIB)

$(BUILD)/%.o: $(CSRC)/%.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# tic_entropy_emb.cpp includes tic_region.cpp, which includes tic_entropy.cpp, which includes
# tic_msssim.cpp, which includes tic_image_batch.cpp, which includes tic_runtime.cpp: the host
# runtime, the image-list entries, the MS-SSIM entries, the entropy coders and the region entries
# are one translation unit (the entries use the handle's internals; tic_runtime.cpp itself stays as
# the shipped tuning states were stamped)
$(BUILD)/tic_entropy_emb.o: $(CSRC)/tic_entropy_emb.cpp $(CSRC)/tic_region.cpp $(CSRC)/tic_entropy.cpp \
                            $(CSRC)/tic_msssim.cpp $(CSRC)/tic_image_batch.cpp $(CSRC)/tic_runtime.cpp $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(BUILD)/range_coder.o: $(CSRC)/range_coder.cpp include/tic.h | $(BUILD)
	g++ -O2 -std=c++17 -fPIC -Wall -Iinclude -c $< -o $@

$(BUILD)/host_util.o: $(CSRC)/host_util.cpp include/tic.h | $(BUILD)
	g++ -O2 -std=c++17 -fPIC -Wall -Iinclude -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS) -Wl,-rpath,/opt/rocm/lib

$(BUILD):
	mkdir -p $(BUILD)

# Host sanitizer build (CPU only): the host C++ that parses user input (range coder,
# CRC-32C of checkpoint bytes) under AddressSanitizer + UBSan, driven by a fuzz harness.
ASAN_BIN := $(BUILD)/host_fuzz_asan
asan: $(ASAN_BIN)
	$(ASAN_BIN) $(BUILD)

$(ASAN_BIN): tests/native/host_fuzz.cpp $(CSRC)/range_coder.cpp $(CSRC)/host_util.cpp include/tic.h | $(BUILD)
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=all \
	    -Iinclude -o $@ tests/native/host_fuzz.cpp $(CSRC)/range_coder.cpp $(CSRC)/host_util.cpp

# The segmented-stream host code (tic_rcseg_*) under the same sanitizers, with its own harness.
RCSEG_BIN := $(BUILD)/rcseg_fuzz_asan
asan-rcseg: $(RCSEG_BIN)
	$(RCSEG_BIN) $(BUILD)

$(RCSEG_BIN): tests/native/rcseg_fuzz.cpp $(CSRC)/range_coder.cpp $(CSRC)/host_util.cpp include/tic.h | $(BUILD)
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=all \
	    -Iinclude -o $@ tests/native/rcseg_fuzz.cpp $(CSRC)/range_coder.cpp $(CSRC)/host_util.cpp

# The version-2 (context) container entries (tic_rcseg_*_ctx; their table CRC is host_util.cpp's).
RCSEG_CTX_BIN := $(BUILD)/rcseg_ctx_fuzz_asan
asan-rcseg-ctx: $(RCSEG_CTX_BIN)
	$(RCSEG_CTX_BIN) $(BUILD)

$(RCSEG_CTX_BIN): tests/native/rcseg_ctx_fuzz.cpp $(CSRC)/range_coder.cpp $(CSRC)/host_util.cpp include/tic.h | $(BUILD)
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=all \
	    -Iinclude -o $@ tests/native/rcseg_ctx_fuzz.cpp $(CSRC)/range_coder.cpp $(CSRC)/host_util.cpp

# The version-3 (causal-neighbour) container entries (tic_rcseg_*_nbr), the same way.
RCSEG_NBR_BIN := $(BUILD)/rcseg_nbr_fuzz_asan
asan-rcseg-nbr: $(RCSEG_NBR_BIN)
	$(RCSEG_NBR_BIN) $(BUILD)

$(RCSEG_NBR_BIN): tests/native/rcseg_nbr_fuzz.cpp $(CSRC)/range_coder.cpp $(CSRC)/host_util.cpp include/tic.h | $(BUILD)
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=all \
	    -Iinclude -o $@ tests/native/rcseg_nbr_fuzz.cpp $(CSRC)/range_coder.cpp $(CSRC)/host_util.cpp

# The symbol-range entries of all three versions (tic_rcseg_range_extent, tic_rcseg_decode_range*).
RCSEG_RANGE_BIN := $(BUILD)/rcseg_range_fuzz_asan
asan-rcseg-range: $(RCSEG_RANGE_BIN)
	$(RCSEG_RANGE_BIN)

$(RCSEG_RANGE_BIN): tests/native/rcseg_range_fuzz.cpp $(CSRC)/range_coder.cpp $(CSRC)/host_util.cpp include/tic.h | $(BUILD)
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=all \
	    -Iinclude -o $@ tests/native/rcseg_range_fuzz.cpp $(CSRC)/range_coder.cpp $(CSRC)/host_util.cpp

# The embedded-table ("TICA") container entries (tic_rcseg_count_nbr, _fit_tables, tic_rcseg_*_emb).
RCSEG_EMB_BIN := $(BUILD)/rcseg_emb_fuzz_asan
asan-rcseg-emb: $(RCSEG_EMB_BIN)
	$(RCSEG_EMB_BIN)

$(RCSEG_EMB_BIN): tests/native/rcseg_emb_fuzz.cpp $(CSRC)/range_coder.cpp $(CSRC)/host_util.cpp include/tic.h | $(BUILD)
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=all \
	    -Iinclude -o $@ tests/native/rcseg_emb_fuzz.cpp $(CSRC)/range_coder.cpp $(CSRC)/host_util.cpp

clean:
	rm -rf $(BUILD) $(LIB)

.PHONY: all clean asan asan-rcseg asan-rcseg-ctx asan-rcseg-nbr asan-rcseg-range asan-rcseg-emb
