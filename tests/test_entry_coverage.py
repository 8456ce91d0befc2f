"""CPU: every entry point that van_gan_amd._lib declares (_SIGS) has a home in the GPU suite.  The convolution variants and the recorded
non-convolution calls of a train step have their own proofs (tests/test_variant_coverage.py, tests/test_call_coverage.py); this file
covers the entry-point list as a whole, by source inspection, so that an entry added without a GPU test fails here.  Three classes:

    1. named literally in a tests/test_gpu_*.py file (the test calls the library directly or through a wrapper it names);
    2. REACHED: a chain from a function of the package whose source names the entry, through callers that each call the link before,
       to a test function of a tests/test_gpu_*.py module -- checked link by link;
    3. UNTESTED_ON_PURPOSE: entries that launch no kernel of the project (host-side queries, thin layers over the runtime's memset and
       copy) or that nothing in the package calls, each with its reason -- and, where the entry still enqueues device work, the
       whole-step test that reaches it.
"""
import ast
import glob
import os
import re

from van_gan_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, 'tests')

# What the direct parity modules tests/test_gpu_rng.py and tests/test_gpu_head.py exist for: these must be class 1, in those files.
DIRECT = {
    'test_gpu_rng': ('vg_randn_bf16', 'vg_dropout_mask', 'vg_randn_bf16_dev', 'vg_dropout_mask_dev'),
    'test_gpu_head': ('vg_dense_head_fwd', 'vg_dense_head_bwd', 'vg_wasserstein_terms', 'vg_bias_grad', 'vg_axpby', 'vg_local_exchange'),
}

# entry -> chain.  A link is 'module:function' ('module:Class.method'); modules of the package are written 'van_gan_amd.x', everything
# else is a file under tests/.  First link: in the package, its source names the entry.  Last link: a test of a test_gpu_* module.
_OPS, _CALLS = 'van_gan_amd.ops:', 'test_gpu_calls:'
_LOSSES = 'test_gpu_calls:test_loss_chain_at_config_shapes'
_SKEL = 'test_gpu_calls:test_skeleton_and_cldice_at_config_shapes'
_CONV = 'test_gpu_ops:test_conv_forward_dgrad_wgrad'
REACHED = {
    'vg_conv3d': (_OPS + 'ConvLayer.forward', _CONV),
    'vg_conv3d_wgrad': (_OPS + 'ConvLayer._wgrad', _OPS + 'ConvLayer.wgrad', _CONV),
    'vg_pack_weights_dma': (_OPS + 'ConvLayer.pack', 'test_gpu_ops:make_layer', _CONV),
    'vg_pack_cell_weights': (_OPS + 'ConvLayer.pack_cell', _OPS + 'ConvLayer.pack', 'test_gpu_ops:make_layer',
                             'test_gpu_ops:test_strided_single_channel_data_gradient_in_cell_form'),
    'vg_pack_up_weights': (_OPS + 'ConvLayer.pack_up', _OPS + 'ConvLayer.pack', 'test_gpu_ops:test_collapsed_upsampled_chunks_of_the_decoder_convolution'),
    'vg_in_finalize': (_OPS + 'in_finalize', _CALLS + 'test_in_finalize_two_sources_and_mult'),
    'vg_actnorm_bwd_stats': (_OPS + 'actnorm_stats', 'test_gpu_ops:test_shortcut_dgrad_concat_norm_fused'),
    'vg_actnorm_bwd_apply': (_OPS + 'actnorm_run', _OPS + 'actnorm_bwd', 'test_gpu_ops:test_in_finalize_and_actnorm_bwd'),
    'vg_actnorm_bwd_apply2': (_OPS + 'actnorm_apply2', 'call_recipes:run_apply2', _CALLS + 'test_apply2_jobs_of_different_grids'),
    'vg_tanh_bwd': (_OPS + 'tanh_bwd', 'test_gpu_ops:test_concat_bwd_and_tanh_bwd'),
    'vg_minmax_apply': (_OPS + 'minmax_apply', _LOSSES),
    'vg_minmax_bwd': (_OPS + 'minmax_bwd', _LOSSES),
    'vg_ssim_fwd': (_OPS + 'ssim_fwd', _LOSSES),
    'vg_ssim_bwd': (_OPS + 'ssim_bwd', _LOSSES),
    'vg_soft_skel_fwd': (_OPS + 'soft_skel_fwd', _SKEL),
    'vg_soft_skel_bwd': (_OPS + 'soft_skel_bwd', _SKEL),
    'vg_cldice_coef': (_OPS + 'cldice_coef', _SKEL),
    'vg_cldice_grads': (_OPS + 'cldice_grads', _SKEL),
    'vg_dot_sums': (_OPS + 'dot_sums', _SKEL),
    'vg_attn_gate_fwd': (_OPS + 'attn_gate_fwd', 'test_gpu_attngate:_gate_kernel_case', 'test_gpu_attngate:test_gate_kernels_at_true_shapes'),
    'vg_attn_gate_bwd': (_OPS + 'attn_gate_bwd', 'test_gpu_attngate:_gate_kernel_case', 'test_gpu_attngate:test_gate_kernels_at_true_shapes'),
    'vg_divide_crop': ('van_gan_amd.inference:stitch_subvolumes', 'test_gpu_inference:test_stitch_subvolumes_matches_oracle'),
    'vg_crop_augment': ('van_gan_amd.data:crop_augment', 'test_gpu_data:test_crop_augment_bit_exact_all_draws'),
    'vg_crop_max': ('van_gan_amd.data:crop_max', 'test_gpu_data:test_crop_max_and_seg_rejection'),
}

# entry -> (kind, reason, whole-step test or None).  kind 'host': the entry enqueues nothing (its definition holds no kernel launch);
# 'unreached': no module of the package calls it; 'runtime': it enqueues device work, but no kernel of the project -- only with the test
# of the whole step that reaches it.
_REPLAY = 'test_gpu_graph:test_launch_list_replay_is_the_eager_step_fp32'
UNTESTED_ON_PURPOSE = {
    'vg_version': ('host', 'returns the ABI version constant', None),
    'vg_abi_sizeof': ('host', 'struct sizes, compared with the ctypes mirrors at load time', None),
    'vg_set_stamp_buffer': ('unreached', 'profiling hook: stores a pointer for the time-stamp builds, no caller in the package', None),
    'vg_conv3d_lds_bytes': ('host', 'LDS bytes of the variant a descriptor would get', None),
    'vg_conv3d_plan': ('host', 'dry run of the dispatch: tile plan of a descriptor', None),
    'vg_conv3d_variant': ('host', 'dry run of the dispatch: name of the kernel variant (tests/test_variant_coverage.py reads it)', None),
    'vg_conv3d_thin_np': ('host', 'channel padding the thin-layer specialist would use', None),
    'vg_conv3d_wgrad_variant': ('host', 'dry run of the weight-gradient dispatch (tests/test_variant_coverage.py reads it)', None),
    'vg_conv3d_dma_bn': ('host', 'column-block width of the LDS-DMA kernels for a descriptor', None),
    'vg_packed_ktot': ('host', 'packed-operand geometry', None),
    'vg_packed_rows': ('host', 'packed-operand geometry', None),
    'vg_value_mode_scratch_bytes': ('host', 'scratch size query', None),
    'vg_spectral_norm_blocks': ('host', 'workgroups per item of a spectral-norm table', None),
    'vg_in_param_grads': ('unreached', 'superseded by the ticketed tail of vg_actnorm_bwd_stats; kept in the ABI, no caller in the package', None),
    'vg_memset_zero': ('runtime', 'hipMemsetAsync under the library\'s stream handle, issued only by a recorded step (ops.zero_fill)', _REPLAY),
    'vg_copy_bytes': ('runtime', 'hipMemcpyAsync under the library\'s stream handle, issued only by a recorded step (ops.copy)', _REPLAY),
}


def _named(name, text):
    return re.search(r'(?<![A-Za-z0-9_])%s(?![A-Za-z0-9_])' % re.escape(name), text) is not None


def _gpu_sources():
    return {os.path.basename(f)[:-3]: open(f).read() for f in sorted(glob.glob(os.path.join(TESTS, 'test_gpu_*.py')))}


_FUNCS = {}


def _source(link):
    """Source text of 'module:function' or 'module:Class.method', cut out of the file (nothing is imported)."""
    mod, qual = link.split(':')
    path = os.path.join(ROOT, *mod.split('.')) + '.py' if mod.startswith('van_gan_amd.') else os.path.join(TESTS, mod + '.py')
    if path not in _FUNCS:
        text = open(path).read()
        table = {}
        for node in ast.parse(text).body:
            if isinstance(node, ast.FunctionDef):
                table[node.name] = ast.get_source_segment(text, node)
            elif isinstance(node, ast.ClassDef):
                for m in node.body:
                    if isinstance(m, ast.FunctionDef):
                        table[node.name + '.' + m.name] = ast.get_source_segment(text, m)
        _FUNCS[path] = table
    assert qual in _FUNCS[path], 'no function %s in %s' % (qual, path)
    return _FUNCS[path][qual]


def _calls(text, link):
    return re.search(r'(?<![A-Za-z0-9_])%s\s*\(' % re.escape(link.split(':')[1].split('.')[-1]), text) is not None


def _is_gpu_test(link):
    mod, qual = link.split(':')
    return mod.startswith('test_gpu_') and qual.startswith('test_') and 'pytest.mark.gpu' in _gpu_sources()[mod] and bool(_source(link))


def test_every_entry_point_has_a_home():
    gpu = _gpu_sources()
    homeless, twice = [], []
    for name in _lib._SIGS:
        literal = any(_named(name, s) for s in gpu.values())
        n = int(literal) + int(name in REACHED) + int(name in UNTESTED_ON_PURPOSE)
        if n == 0:
            homeless.append(name)
        if name in UNTESTED_ON_PURPOSE and (literal or name in REACHED):
            twice.append(name)                          # an entry with a test is not untested on purpose
    assert not homeless, 'entry points without a GPU test (name them in a tests/test_gpu_*.py file or list them here): %s' % homeless
    assert not twice, twice
    stale = [n for n in list(REACHED) + list(UNTESTED_ON_PURPOSE) if n not in _lib._SIGS]
    assert not stale, stale
    assert len(_lib._SIGS) >= 89


def test_the_direct_parity_modules_name_their_entries():
    gpu = _gpu_sources()
    for mod, names in DIRECT.items():
        for name in names:
            assert name in _lib._SIGS and _named(name, gpu[mod]), (mod, name)
            assert name not in UNTESTED_ON_PURPOSE and name not in REACHED, name


def test_reached_chains_hold_link_by_link():
    for name, chain in REACHED.items():
        assert len(chain) >= 2 and chain[0].startswith('van_gan_amd.'), name
        assert _named(name, _source(chain[0])), '%s does not name %s' % (chain[0], name)
        for callee, caller in zip(chain, chain[1:]):
            assert _calls(_source(caller), callee), '%s: %s does not call %s' % (name, caller, callee)
        assert _is_gpu_test(chain[-1]), (name, chain[-1])


def _definition(name):
    """Body of the extern "C" definition of an entry in the HIP sources."""
    for f in sorted(glob.glob(os.path.join(ROOT, 'van_gan_amd', 'csrc', '*.hip'))):
        text = open(f).read()
        m = re.search(r'extern "C" [^;{]*?(?<![A-Za-z0-9_])%s\s*\([^;{]*\)\s*\{' % re.escape(name), text)
        if m:
            depth, i = 1, m.end()
            while depth:
                depth += {'{': 1, '}': -1}.get(text[i], 0)
                i += 1
            return text[m.end():i]
    raise AssertionError('no definition of %s' % name)


def test_untested_entries_are_what_their_reason_says():
    package = {f: open(f).read() for f in glob.glob(os.path.join(ROOT, 'van_gan_amd', '*.py')) if not f.endswith('_lib.py')}
    for name, (kind, reason, test) in UNTESTED_ON_PURPOSE.items():
        assert kind in ('host', 'unreached', 'runtime') and reason, name
        body = _definition(name)
        if kind == 'host':
            assert not re.search(r'hipLaunchKernelGGL|<<<|hipMemsetAsync|hipMemcpyAsync', body), name
        if kind == 'unreached':
            assert not [f for f, s in package.items() if _named(name, s)], name
        if kind == 'runtime':
            assert not re.search(r'hipLaunchKernelGGL|<<<', body), name
        if kind == 'runtime':
            assert test is not None and _is_gpu_test(test), name
        else:
            assert test is None, name
