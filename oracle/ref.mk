# Builds the reference's own GPU code for gfx950 (test infrastructure): oracle/_ref/libref_c0.so and libref_c1.so, which
# tests/test_gpu_reference.py runs next to the product.  Output and intermediates stay in oracle/_ref/ (git-ignored); nothing of the
# reference is committed.  Driven by oracle.build_ref(), which passes REF (the reference tree: src/*.cu and include/*.h are read).
#
# Translation: hipify-perl, then two generic text fix-ups -- strip a UTF-8 byte-order mark wherever hipify left it, and close up
# launch chevrons written with spaces ("<< <grid, block >> >" -> "<<<grid, block >>>").
# Flags: -fhip-fp32-correctly-rounded-divide-sqrt and -fno-gpu-flush-denormals-to-zero are nvcc's defaults (-prec-div=true,
# -ftz=false) spelled out.  c0 contracts nothing (RTDD_OPT_FP_CONTRACT = 0); c1 fuses every a*b+c the source writes
# (RTDD_OPT_FP_CONTRACT = 1) -- without -fno-slp-vectorize the SLP vectorizer pairs the solver's sum/count additions into
# v_pk_add_f32 first and leaves those four products unfused.  -Wl,-Bsymbolic: librtdd.so exports the same ten mangled names, and
# the reference's calls into itself must bind to its own code.
ifndef REF
$(error REF=<reference tree> is required)
endif
HIPIFY  ?= /opt/rocm/bin/hipify-perl
HIPCC   ?= /opt/rocm/bin/hipcc
OUT     := _ref
NAMES   := GPUSolver GPUImageProcessing GPUDepthEffect
HIPS    := $(NAMES:%=$(OUT)/%.hip)
FLAGS   := -O3 --offload-arch=gfx950 -fhip-fp32-correctly-rounded-divide-sqrt -fno-gpu-flush-denormals-to-zero -fPIC -shared \
           -Wl,-Bsymbolic -w -I$(REF)/include
C0      := -ffp-contract=off
C1      := -ffp-contract=fast -fno-slp-vectorize

all: $(OUT)/libref_c0.so $(OUT)/libref_c1.so

$(OUT)/%.hip: $(REF)/src/%.cu ref.mk
	@mkdir -p $(OUT)
	$(HIPIFY) $< > $@.tmp 2> $@.log
	sed -e 's/\xEF\xBB\xBF//' -e 's/<< *<\([^<>]*\)>> *>/<<<\1>>>/g' $@.tmp > $@
	rm -f $@.tmp

$(OUT)/libref_c0.so: $(HIPS) $(wildcard $(REF)/include/*.h)
	$(HIPCC) $(FLAGS) $(C0) -o $@ $(HIPS)

$(OUT)/libref_c1.so: $(HIPS) $(wildcard $(REF)/include/*.h)
	$(HIPCC) $(FLAGS) $(C1) -o $@ $(HIPS)

# echoes the compile line of one variant (tests/test_reference_build.py reruns it with -S to read the ISA)
print-flags-%:
	@echo $(FLAGS) $($*)

.PHONY: all print-flags-%
