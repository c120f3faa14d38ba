"""The training drivers' loop (reference train.py:25-134 and train_multi_attr.py:43-231), single process or one
process per GPU.  Call order per iteration is the reference's: get_w -> get_logits -> get_reg_preds -> get_train_alpha ->
get_alphas -> get_w_new_tensor -> get_logits -> optimizeParametersAll (graph.TransformGraph.eager_step; the PGGAN graph's is
pggan.walk_training_step).  Under data parallelism every rank draws the same
z (seed = epoch) and the same alpha (same numpy seed) and takes every world-th sample of the batch (dist.shard: strided shards keep the discriminator's stddev groups whole)."""
import logging
import math
import os
import time

import numpy as np

from . import constants, dist, hostutil


def _configure_logging(path, append=False):
    root = logging.getLogger()
    root.setLevel(logging.INFO)
    for h in list(root.handlers):
        root.removeHandler(h)
    fmt = logging.Formatter('%(asctime)s %(levelname)s %(message)s')
    fh = logging.FileHandler(path, mode='a' if append else 'w')
    fh.setFormatter(fmt)
    root.addHandler(fh)
    sh = logging.StreamHandler()
    sh.setFormatter(fmt)
    root.addHandler(sh)


def make_samples(img_tensor, output_dir, epoch, optim_iter, batch_size, pre_path='results', name='test'):
    """PNG grid of a batch (train.py:137-144), every save_freq iterations.  A batch on the GPU is quantised and laid out there by one
    l2i_panels_u8 launch and crosses to the host as the finished uint8 grid (1 byte a value instead of 4, no numpy pass on the training thread);
    a CPU tensor, or a library without that entry point, takes the host path.  The same pixels either way."""
    from PIL import Image
    from . import _lib
    cols = max(int(math.sqrt(batch_size)), 1)
    rows = (img_tensor.shape[0] + cols - 1) // cols
    path = '{}/{}/{}_{}_{}.png'.format(output_dir, pre_path, epoch, optim_iter, name)
    if img_tensor.is_cuda and img_tensor.shape[1] == 3 and _lib.has('l2i_panels_u8'):
        from . import kernels
        grid = kernels.panels_u8(img_tensor.detach().float(), range(rows * cols), 1, rows, cols, pad=0, fill=0)[0].cpu().numpy()
        Image.fromarray(grid).save(path)
        return
    img = img_tensor.detach().cpu().numpy()
    img = np.uint8(np.clip(((img + 1) / 2.0) * 255, 0, 255)).transpose(0, 2, 3, 1)
    h, w = img.shape[1], img.shape[2]
    grid = np.zeros((rows * h, cols * w, 3), np.uint8)
    for i in range(img.shape[0]):
        r, c = divmod(i, cols)
        grid[r * h:(r + 1) * h, c * w:(c + 1) * w] = img[i]
    Image.fromarray(grid).save(path)


def train_step(graphs, zs_batch, attrList, layers=None, trainEmbed=False, updateGAN=False, opt=None, multi_attr=False):
    """One iteration of the hot loop.  ``zs_batch``: this rank's [B_local, 512] numpy slice.  The alpha of the step is drawn here, once, from the
    global numpy RNG (for the PGGAN graph it is the delta of train_multi_attr.py:113's clamp pair); the graph runs the step, call by call
    (``eager_step``) or, under --hip_graph, recorded once and replayed (``captured_step``): full batches replay, a ragged last batch, trainEmbed and
    a step the graph does not record (the PGGAN graph's GAN term, which raises) or recorded with other flags run eagerly.
    Returns (loss tensor, alpha_for_target, out_zs, transformed_output)."""
    hip_graph = opt is not None and getattr(opt, 'hip_graph', False)
    if hip_graph and not hasattr(graphs, 'captured_step'):
        raise NotImplementedError('--hip_graph records the StyleGAN2 step (capture.CapturedStep) or the PGGAN z-walk step (capture.CapturedZStep); '
                                  'this graph offers neither')
    flags = dict(clamp=multi_attr, layers=layers, no_content_loss=bool(opt and opt.no_content_loss), no_gan_loss=bool(opt and opt.no_gan_loss))
    alpha_for_graph, alpha_for_target, _ = graphs.get_train_alpha(zs_batch, N_attr=len(attrList), trainEmbed=trainEmbed)
    if hip_graph and not trainEmbed and zs_batch.shape[0] == _captured_batch(graphs, zs_batch.shape[0], len(attrList), flags):
        r = graphs._captured_step(zs_batch, alpha_for_graph)
        return r['loss'], alpha_for_target, r['x0'], r['x1']
    loss, out_zs, transformed_output = graphs.eager_step(zs_batch, alpha_for_graph, trainEmbed=trainEmbed, updateGAN=updateGAN, **flags)
    return loss, alpha_for_target, out_zs, transformed_output


def _captured_batch(graphs, batch, n_attr, flags):
    """The batch size of the graph's recorded step, built on first use (the local batch size and the flags are static from then on); None when the
    graph does not record a step with these flags, or recorded it with others."""
    st = getattr(graphs, '_captured_step', None)
    if st is None:
        st = graphs._captured_step = graphs.captured_step(batch, n_attr, **flags)
        if st is not None:
            st.flags = flags
    return None if st is None or st.flags != flags else st.z.shape[0]


def train(graphs, graph_inputs, output_dir, attrList, layers=None, save_freq=100, trainEmbed=False, updateGAN=False,
          opt=None, multi_attr=False):
    """train.py:25-134.  Side effect on the host process, undone on return: after the first step every Python object alive is moved to the
    garbage collector's permanent generation (``gc.freeze``: a full collection over the networks' ~270 000 host objects takes 73 ms on the thread
    that launches the step's kernels); ``gc.unfreeze()`` runs in a ``finally`` when training ends, so a caller that drops
    this graph and builds another (notebooks, eval, tests) keeps a working cycle collector.  ``opt.no_gc_freeze`` switches the freeze off."""
    from . import nets16
    watch, keep = int(getattr(opt, 'f16_watch', 0) or 0) if opt is not None else 0, nets16.MONITOR
    try:
        if watch:
            # --f16_watch: a range monitor behind the probe points of the 16-bit networks for the whole run (set before the step is captured, so
            # that under --hip_graph its launches are part of the recorded step); read, logged and cleared every `watch` iterations in _train
            nets16.MONITOR = nets16.RangeMonitor(graphs.device)
        return _train(graphs, graph_inputs, output_dir, attrList, layers, save_freq, trainEmbed, updateGAN, opt, multi_attr)
    finally:
        nets16.MONITOR = keep
        import gc
        gc.unfreeze()


def _log_ranges(monitor, is_main):
    """One --f16_watch report: read the monitor (the host synchronisation of the flag), log nets16.watch_report's lines, clear it."""
    from . import nets16
    if is_main:
        for level, text in nets16.watch_report(monitor.read()):
            (logging.warning if level == 'warning' else logging.info)(text)
    monitor.clear()


def _train(graphs, graph_inputs, output_dir, attrList, layers, save_freq, trainEmbed, updateGAN, opt, multi_attr):
    is_main = dist.rank() == 0
    if is_main:
        os.makedirs(os.path.join(output_dir, 'results'), exist_ok=True)
        _configure_logging(os.path.join(output_dir, 'log.txt'), append=False)
        logging.info('weight sources: {}'.format(getattr(graphs, 'weight_sources', None)))
    n_epoch = (opt.n_epoch if opt is not None and getattr(opt, 'n_epoch', None) else (3 if multi_attr else 10))
    batch_size = constants.BATCH_SIZE
    num_samples = graph_inputs['z'].shape[0]
    sl = dist.shard(batch_size)
    sync_log = not (opt is not None and getattr(opt, 'no_log_sync', False))
    loss_values = []
    from . import nets16
    watch, done = (int(getattr(opt, 'f16_watch', 0) or 0) if opt is not None and nets16.MONITOR is not None else 0), 0
    for epoch in range(n_epoch):
        if updateGAN:
            raise NotImplementedError('ERROR: jointly training is not implemented yet')      # train.py:40-41
        iters = num_samples // batch_size
        if opt is not None and getattr(opt, 'max_iters', None):
            iters = min(iters, opt.max_iters)
        graph_inputs = hostutil.graph_input(graphs, num_samples, seed=epoch)                 # train.py:45
        print('Number of the training epochs and iterations: ', n_epoch, iters)
        for i in range(iters):
            batch_start = i * batch_size
            start_time = time.time()
            s = slice(batch_start, min(num_samples, batch_start + batch_size))
            zs_batch = hostutil.batch_input(graph_inputs, s)['z'][sl]
            loss, at, out_zs, transformed = train_step(graphs, zs_batch, attrList, layers, trainEmbed, updateGAN, opt, multi_attr)
            if epoch == 0 and i == 0 and not (opt is not None and getattr(opt, 'no_gc_freeze', False)):
                from . import capture
                capture.freeze_host_objects()                 # everything built lazily by the first step is long-lived: out of the collector's way
            if sync_log:
                curr = loss.detach().cpu().item()                                             # train.py:110
                loss_values.append(curr)
                if is_main:
                    logging.info('T, epc, bst, lss, alpha: {}, {}, {}, {}, {}'.format(
                        time.time() - start_time, epoch, batch_start, loss, round(float(at[0]), 2)))
            done += 1
            if watch and done % watch == 0:
                _log_ranges(nets16.MONITOR, is_main)
            if is_main and (i % save_freq == 0):
                make_samples(out_zs, output_dir, epoch, i * batch_size, batch_size, name='org_%.2f' % (round(float(at[0]), 2)))
                make_samples(transformed, output_dir, epoch, i * batch_size, batch_size, name='logit_%.2f' % (round(float(at[0]), 2)))
        graphs.save_multi_models('{}/model_w_{}'.format(output_dir, epoch), '{}/model_gan_{}.ckpt'.format(output_dir, epoch),
                                 trainEmbed=trainEmbed, updateGAN=updateGAN)
    graphs.save_multi_models('{}/model_w_{}_final'.format(output_dir, n_epoch), '{}/model_gan_{}_final.ckpt'.format(output_dir, n_epoch),
                             trainEmbed=trainEmbed, updateGAN=updateGAN)
    if multi_attr and is_main and loss_values:
        np.save(os.path.join(output_dir, 'loss_values.npy'), np.asarray(loss_values))        # train_multi_attr.py:226-231
    return loss_values


def main(multi_attr=False, argv=None):
    from . import graph as graph_mod
    from .options import TrainOptions
    opt = TrainOptions().parse(print_opt=(int(os.environ.get('RANK', '0')) == 0), argv=argv)
    dist.select_gpu(opt.gpu)                         # train.py:150 — before the first torch.cuda call (init_from_env makes it)
    rk, world, local = dist.init_from_env()
    dist.assert_distinct_devices()                   # N ranks over RCCL must sit on N distinct physical GPUs
    if opt.synthetic_weights:
        constants.ALLOW_SYNTHETIC_WEIGHTS = True
    if opt.precision:
        from . import conv
        conv.PRECISION = opt.precision
    if opt.resolution:
        constants.resolution = opt.resolution
    if opt.batch_size:
        constants.BATCH_SIZE = opt.batch_size
    if opt.seed is not None:
        np.random.seed(opt.seed)
    elif world > 1:
        np.random.seed(1234)                         # identical walk init and alpha stream on every rank
    graph_kwargs = hostutil.set_graph_kwargs(opt)
    model = graph_mod.find_model_using_name(opt.model, opt.transform)
    from . import nets16
    nets16.F16_SCALES_FLAG = getattr(opt, 'f16_scales', None)      # --f16_scales: read where the graph builds its LossScaler (nets16.loss_scale_for)
    try:
        g = model(**graph_kwargs)
    finally:
        nets16.F16_SCALES_FLAG = None
    if getattr(g, 'id_weight', 0.0):                 # --id_loss: the face network now, so that a missing checkpoint stops the run here and its source is recorded
        g.check_id_loss()
        g.face_net()
    if getattr(g, 'attr_keep', 0.0) and rk == 0:     # --attr_keep: which regressor outputs the walk is trained to hold still
        print('attribute-preservation term: weight %g over %d regressor outputs %s' % (g.attr_keep, len(g.keepIdx), list(g.keepIdx)))
    if world > 1:                                    # one source of truth for the trainable state
        dist.broadcast_parameters(g.walk.parameters())
    if getattr(opt, 'f16_calibrate', 0):             # before the first step and the first capture: a recorded graph has the static scales baked in
        rec = g.calibrate_scales(opt.f16_calibrate, clamp=multi_attr, layers=graph_kwargs['layers'], no_content_loss=bool(opt.no_content_loss),
                                 no_gan_loss=bool(opt.no_gan_loss))
        if rk == 0:
            import json
            print('fp16 gradient scales: table / flags %s -> calibrated %s (%d rounds of %d probe steps)' % (rec['start'], rec['chosen'], rec['rounds'], opt.f16_calibrate))
            with open(os.path.join(opt.output_dir, 'f16_scales.json'), 'wt') as f:
                json.dump(dict(start=rec['start'], chosen=rec['chosen'], rounds=rec['rounds'], probe_steps=opt.f16_calibrate, tags=rec['tags']), f, indent=1, sort_keys=True)
                f.write('\n')
    if rk == 0:                                      # which frozen weights this run trained against: stdout, opt.yml (and log.txt in train())
        print('weight sources: ', g.weight_sources)
        yml = os.path.join(opt.output_dir, 'opt.yml')
        if os.path.isfile(yml):
            import yaml
            with open(yml) as f:
                dump = yaml.load(f, Loader=yaml.FullLoader)
            dump['weight_sources'] = dict(g.weight_sources)
            with open(yml, 'wt') as f:
                yaml.dump(dump, f, default_flow_style=False)
    graph_inputs = hostutil.graph_input(g, opt.num_samples, seed=0)
    attrList = graph_kwargs['attrList']
    print('attrlist: ', attrList)
    train(g, graph_inputs, opt.output_dir, attrList, layers=graph_kwargs['layers'], save_freq=opt.model_save_freq,
          trainEmbed=opt.trainEmbed, updateGAN=opt.updateGAN, opt=opt, multi_attr=multi_attr)
