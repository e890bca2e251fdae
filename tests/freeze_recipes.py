"""The reference's freeze recipes as functions on a built model, for the GPU step tests (test_gpu_freeze_recipes.py).

`--timesformer-freeze-space` (models.py:320-349 of the reference) freezes every parameter of the video tower that the OpenAI
CLIP checkpoint supplied -- the names `remap_keys` makes of the ViT's state dict -- except cls_token, and trains the rest
(temporal_embed, timeattn, norm3). The names are derived here from `remap_keys` itself on a key list of the ViT's layout, so
that no CLIP file is needed; test_freeze_cases_cpu.py pins the result against the flags the reference's constructor left
(tests/golden/reference_boundary.pt, pretrained_clip['512-True']['requires_grad'])."""
_VIT_TOP_KEYS = ('class_embedding', 'positional_embedding', 'proj', 'conv1.weight', 'ln_pre.weight', 'ln_pre.bias',
                 'ln_post.weight', 'ln_post.bias')
_VIT_BLOCK_KEYS = ('attn.in_proj_weight', 'attn.in_proj_bias', 'attn.out_proj.weight', 'attn.out_proj.bias', 'ln_1.weight',
                   'ln_1.bias', 'ln_2.weight', 'ln_2.bias', 'mlp.c_fc.weight', 'mlp.c_fc.bias', 'mlp.c_proj.weight',
                   'mlp.c_proj.bias')


def clip_supplied_names(depth):
    """Names (inside the video tower) of the parameters a CLIP ViT of `depth` layers supplies."""
    import torch
    from lavila.models.utils import remap_keys
    z = torch.zeros(1)
    sd = {k: z for k in _VIT_TOP_KEYS}
    sd.update({f'transformer.resblocks.{i}.{k}': z for i in range(depth) for k in _VIT_BLOCK_KEYS})
    return set(remap_keys(sd, transformer_layers=depth).keys())


def freeze_space_flags(param_names, depth):
    """{name: requires_grad} of the timesformer_freeze_space pattern for the tower's parameter names."""
    supplied = clip_supplied_names(depth)
    return {n: (n not in supplied or n == 'cls_token') for n in param_names}


def apply_freeze_space(vis):
    flags = freeze_space_flags([n for n, _ in vis.named_parameters()], len(vis.blocks))
    for n, p in vis.named_parameters():
        p.requires_grad = flags[n]
    return flags


def apply_recipe(vis, recipe):
    """recipe: 'spatial' (freeze_spatial_weights), 'temporal' (freeze_temporal_weights), 'freeze_space' or 'none'."""
    import contextlib
    import io
    for p in vis.parameters():
        p.requires_grad = True
    with contextlib.redirect_stdout(io.StringIO()):
        if recipe == 'spatial':
            vis.freeze_spatial_weights()
        elif recipe == 'temporal':
            vis.freeze_temporal_weights()
        elif recipe == 'freeze_space':
            apply_freeze_space(vis)
        elif recipe != 'none':
            raise ValueError(recipe)
    return {n: p.requires_grad for n, p in vis.named_parameters()}


VIDEO_RECIPES = ('spatial', 'temporal', 'freeze_space')

# (b) of the recipe tests: results of a frozen step that need NOT equal the unfrozen step's bit for bit: {recipe: {parameter-name
# pattern: the kernel instantiation the frozen run does not share}}; the pattern '' is every parameter and the loss.
# One entry. With the narrator's tower fully frozen nothing in the tower wants a gradient, and ops.linear then takes its
# inference route for widths lvl_linear_tn does not tile both ways: the 192-wide tower of the golden narrator runs its Linears
# on lvl_linear_skinny (fc1, whose forward alone tiles, on lvl_linear_tn by _LinearFn's `own` rule) where every step with a
# trainable tower runs them on the library GEMM. The tower's output, and with it the loss and every gradient behind it, differs in
# rounding; which of the two kernels rounds differently is not isolated (the patch embedding alone, which freeze_spatial_weights
# moves to lvl_linear_skinny too, stays bit-equal). At the widths of the published towers (768 / 1024) both steps run
# lvl_linear_tn. Every other recipe gives the same bits for every gradient it still wants.
BITWISE_EXCEPTIONS = {
    'narrator lm+visual+visual_temporal': {'': 'lvl_linear_skinny / lvl_linear_tn (ops.linear and _LinearFn without gradients, '
                                               '192-wide tower) where the steps with a trainable tower run the library GEMM'},
}
